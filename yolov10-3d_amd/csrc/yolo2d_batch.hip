// 2D training batches on the device: the image and label work of YOLODataset.__getitem__ (data/base.py:147-182, 251-266;
// data/augment.py v8_transforms :973-1007, Format :915-957) and collate_fn (data/dataset.py:206-223).  Host code (yolo2d.py) reads the
// files and draws every random number; two kernels do the rest.
//
// y3d_yolo2d_image_aug — one launch per batch, one thread per FOUR neighbouring output pixels of a row.  Only the float mode stores
// 16 bytes at a time (one float4 per channel plane); the uint8 mode writes the thread's 12 contiguous bytes of the channels-last image
// as three 4-byte words.  The contents of rec_i are trusted once yolo2d.pack_images has checked them on the host (a caller that
// rewrites the records on the device, as a graph replay does, answers for them): a tile whose source index or sizes are out of
// range is not read and gives 114, it raises nothing.  Each output pixel is computed
// backwards; every coordinate and weight is float64 with contraction off, and only + - * / and floor are used, in this order:
//
//   1. un-flip:   ux = fliplr ? S-1-ox : ox,  uy = flipud ? S-1-oy : oy                (RandomFlip; a permutation, so it commutes)
//   2. per layer (0: the sample, 1: its MixUp partner), with the layer's inverse matrix i (float64, output -> canvas):
//        sx = (i0*ux + i1*uy) + i2,  sy = (i3*ux + i4*uy) + i5
//        not (-1 < sx < C and -1 < sy < C)  ->  114                                    (C: canvas side, 2S mosaic / S letter-box)
//        x0 = floor(sx), ax = sx - x0,  y0 = floor(sy), ay = sy - y0
//        w = ((c00*(1-ax) + c01*ax)*(1-ay)) + ((c10*(1-ax) + c11*ax)*ay),  cjk = canvas(x0+k, y0+j);   warped = floor(w + 0.5)
//      canvas(cx, cy) = 114 outside [0, C)^2 or when no tile rectangle [x1a, x2a) x [y1a, y2a) holds it, else tile(cx-padw, cy-padh)
//      tile(tx, ty)   = the source pixel itself when the tile was not resized (h == h0 and w == w0), else
//        fx = (tx + 0.5)*(w0/w) - 0.5,  X0 = floor(fx), bx = fx - X0;  X0 < 0 -> (0, bx 0);  X0 >= w0-1 -> (w0-1, bx 0);  same in y
//        v = ((p00*(1-bx) + p01*bx)*(1-by)) + ((p10*(1-bx) + p11*bx)*by);   tile = floor(v + 0.5)
//   3. MixUp:     m = floor(warped0*r + warped1*(1-r))                                 (numpy's astype(uint8) truncates)
//   4. HSV (when any gain is non-zero), channels named r, g, b:
//        V = max, d = V - min,  Sat = V == 0 ? 0 : floor(255*d/V + 0.5)
//        hdeg = d == 0 ? 0 : V == r ? 60*(g-b)/d : V == g ? 120 + 60*(b-r)/d : 240 + 60*(r-g)/d;  hdeg < 0 -> hdeg + 360
//        H = floor(hdeg/2 + 0.5);  H >= 180 -> H - 180;      H', S', V' = lutH[H], lutS[Sat], lutV[V]
//        hh = H'/30, i = floor(hh), f = hh - i, s = S'/255;  p = V'*(1-s), q = V'*(1-s*f), t = V'*(1-s*(1-f))
//        (r, g, b) = i: 0 (V',t,p) 1 (q,V',p) 2 (p,V',t) 3 (p,q,V') 4 (t,p,V') 5 (V',p,q);  each floor(. + 0.5)
//   5. channel order (Format's bgr draw) and layout: mode 0 (B, 3, S, S) float32 = value / 255, mode 1 (B, S, S, 3) uint8.
//
// A tap whose weight is exactly zero is not loaded (its product is an exact zero either way).  tests/yolo2d_ref.py states the same
// arithmetic in numpy float64; it is not OpenCV's fixed-point resize / warp nor its integer HSV tables.
//
// y3d_yolo2d_encode_labels — one workgroup of 256 lanes per output image; the candidates (boxes of mosaic tiles 0..3, then of the
// partner's 0..3) are walked in chunks of 256, one box per lane, in float32 as numpy computes them, then compacted in order: ballot +
// popcount within a wave, an LDS prefix over the four waves, a running base across chunks.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int YI_TILE = 12;   // src, h0, w0, h, w, x1a, y1a, x2a, y2a, padw, padh, 0
constexpr int YI_LAYER = 2 + 4 * YI_TILE;  // tiles, canvas side, four tiles
constexpr int YI_REC = 112;   // two layers, then flipud, fliplr, bgr, hsv, mix
constexpr int YI_F = 16;      // inverse matrix of layer 0 (6), of layer 1 (6), r
constexpr int YL_I = 20;      // (start, n) of eight tiles, flags of the two layers, flips, 0
constexpr int YL_F = 48;      // (w, h, padw, padh) of eight tiles, (M 2x3, scale, 0) of the two layers

struct ImgP {
  const unsigned char* const* src;
  int n_src;
  const int* rec_i;
  const double* rec_f;
  const unsigned char* lut;
  int S, mode;
};

__device__ __forceinline__ double lerp2(double p00, double p01, double p10, double p11, double ax, double ay) {
  return ((p00 * (1.0 - ax) + p01 * ax) * (1.0 - ay)) + ((p10 * (1.0 - ax) + p11 * ax) * ay);
}

// a pixel of the tile = the source image resized to (h, w)
__device__ __forceinline__ void tile_px(const unsigned char* __restrict__ p, int h0, int w0, int h, int w, int ty, int tx, double v[3]) {
  ty = min(max(ty, 0), h - 1);
  tx = min(max(tx, 0), w - 1);
  if (h == h0 && w == w0) {
    const unsigned char* q = p + ((size_t)ty * w0 + tx) * 3;
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
    return;
  }
  const double fx = ((double)tx + 0.5) * ((double)w0 / (double)w) - 0.5;
  const double fy = ((double)ty + 0.5) * ((double)h0 / (double)h) - 0.5;
  const double xf = floor(fx), yf = floor(fy);
  double bx = fx - xf, by = fy - yf;
  int x0 = (int)xf, y0 = (int)yf;
  if (x0 < 0) { x0 = 0; bx = 0.0; }
  if (x0 >= w0 - 1) { x0 = w0 - 1; bx = 0.0; }
  if (y0 < 0) { y0 = 0; by = 0.0; }
  if (y0 >= h0 - 1) { y0 = h0 - 1; by = 0.0; }
  const int x1 = min(x0 + 1, w0 - 1), y1 = min(y0 + 1, h0 - 1);
  const unsigned char* r0 = p + (size_t)y0 * w0 * 3;
  const unsigned char* r1 = p + (size_t)y1 * w0 * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    v[c] = floor(lerp2((double)r0[x0 * 3 + c], (double)r0[x1 * 3 + c], (double)r1[x0 * 3 + c], (double)r1[x1 * 3 + c], bx, by) + 0.5);
}

__device__ __forceinline__ void canvas_px(const ImgP& P, const int* __restrict__ L, int cx, int cy, double v[3]) {
  v[0] = v[1] = v[2] = 114.0;
  const int C = L[1];
  if (cx < 0 || cy < 0 || cx >= C || cy >= C) return;
  int k = -1;
  const int nt = min(L[0], 4);
  for (int t = 0; t < nt; ++t) {
    const int* T = L + 2 + t * YI_TILE;
    const bool in = cx >= T[5] && cx < T[7] && cy >= T[6] && cy < T[8];
    k = in ? t : k;
  }
  if (k < 0) return;
  const int* T = L + 2 + k * YI_TILE;
  const int s = T[0];
  if (s < 0 || s >= P.n_src || T[1] < 1 || T[2] < 1 || T[3] < 1 || T[4] < 1) return;
  tile_px(P.src[s], T[1], T[2], T[3], T[4], cy - T[10], cx - T[9], v);
}

__device__ __forceinline__ void warp_px(const ImgP& P, const int* __restrict__ L, const double* __restrict__ iv, double ux, double uy,
                                        double v[3]) {
  const double C = (double)L[1];
  const double sx = (iv[0] * ux + iv[1] * uy) + iv[2];
  const double sy = (iv[3] * ux + iv[4] * uy) + iv[5];
  if (!(sx > -1.0 && sx < C && sy > -1.0 && sy < C)) {
    v[0] = v[1] = v[2] = 114.0;
    return;
  }
  const double xf = floor(sx), yf = floor(sy);
  const double ax = sx - xf, ay = sy - yf;
  const int x0 = (int)xf, y0 = (int)yf;
  double c00[3], c01[3] = {0, 0, 0}, c10[3] = {0, 0, 0}, c11[3] = {0, 0, 0};
  canvas_px(P, L, x0, y0, c00);
  if (ax != 0.0) canvas_px(P, L, x0 + 1, y0, c01);
  if (ay != 0.0) {
    canvas_px(P, L, x0, y0 + 1, c10);
    if (ax != 0.0) canvas_px(P, L, x0 + 1, y0 + 1, c11);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = floor(lerp2(c00[c], c01[c], c10[c], c11[c], ax, ay) + 0.5);
}

__device__ __forceinline__ void hsv_px(const unsigned char* __restrict__ lut, double v[3]) {
  const double r = v[0], g = v[1], b = v[2];
  const double V = fmax(r, fmax(g, b)), mn = fmin(r, fmin(g, b));
  const double d = V - mn;
  const double Sat = V == 0.0 ? 0.0 : floor(255.0 * d / V + 0.5);
  double hdeg = d == 0.0 ? 0.0 : V == r ? 60.0 * (g - b) / d : V == g ? 120.0 + 60.0 * (b - r) / d : 240.0 + 60.0 * (r - g) / d;
  if (hdeg < 0.0) hdeg = hdeg + 360.0;
  double H = floor(hdeg / 2.0 + 0.5);
  if (H >= 180.0) H = H - 180.0;
  const double H2 = (double)lut[min(max((int)H, 0), 255)];
  const double S2 = (double)lut[256 + min(max((int)Sat, 0), 255)];
  const double V2 = (double)lut[512 + min(max((int)V, 0), 255)];
  const double hh = H2 / 30.0;
  const double fi = floor(hh);
  const double f = hh - fi;
  const double s = S2 / 255.0;
  const double p = V2 * (1.0 - s), q = V2 * (1.0 - s * f), t = V2 * (1.0 - s * (1.0 - f));
  int i = (int)fi;
  if (i > 5) i -= 6;
  const double R = i == 0 ? V2 : i == 1 ? q : i == 2 ? p : i == 3 ? p : i == 4 ? t : V2;
  const double G = i == 0 ? t : i == 1 ? V2 : i == 2 ? V2 : i == 3 ? q : i == 4 ? p : p;
  const double Bc = i == 0 ? p : i == 1 ? p : i == 2 ? t : i == 3 ? V2 : i == 4 ? V2 : q;
  v[0] = floor(R + 0.5);
  v[1] = floor(G + 0.5);
  v[2] = floor(Bc + 0.5);
}

__global__ void __launch_bounds__(256) yolo2d_image_kernel(ImgP P, void* __restrict__ out) {
  const int S = P.S;
  const int b = blockIdx.y;
  const int groups = S >> 2;  // S % 4 == 0 (checked by the entry)
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= S * groups) return;
  const int oy = g / groups, ox4 = (g - oy * groups) * 4;
  const int* ri = P.rec_i + (size_t)b * YI_REC;
  const double* rf = P.rec_f + (size_t)b * YI_F;
  const int flipud = ri[100], fliplr = ri[101], bgr = ri[102], hsv = ri[103], mix = ri[104];
  const double r = rf[12];
  const unsigned char* lut = P.lut + (size_t)b * 768;
  const double uy = (double)(flipud ? S - 1 - oy : oy);
  unsigned res[12];  // four pixels x three channels, in the output's channel order
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ox = ox4 + j;
    const double ux = (double)(fliplr ? S - 1 - ox : ox);
    double v[3];
    warp_px(P, ri, rf, ux, uy, v);
    if (mix) {
      double v2[3];
      warp_px(P, ri + YI_LAYER, rf + 6, ux, uy, v2);
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = floor(v[c] * r + v2[c] * (1.0 - r));
    }
    if (hsv) hsv_px(lut, v);
    const double c0 = bgr ? v[2] : v[0], c2 = bgr ? v[0] : v[2];
    res[j * 3 + 0] = (unsigned)fmin(fmax(c0, 0.0), 255.0);
    res[j * 3 + 1] = (unsigned)fmin(fmax(v[1], 0.0), 255.0);
    res[j * 3 + 2] = (unsigned)fmin(fmax(c2, 0.0), 255.0);
  }
  if (P.mode == 0) {
    float* o = (float*)out;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float4 q = make_float4((float)res[c] / 255.f, (float)res[3 + c] / 255.f, (float)res[6 + c] / 255.f, (float)res[9 + c] / 255.f);
      *(float4*)(o + (((size_t)b * 3 + c) * S + oy) * S + ox4) = q;
    }
  } else {
    unsigned* o = (unsigned*)((unsigned char*)out + (((size_t)b * S + oy) * S + ox4) * 3);
#pragma unroll
    for (int w = 0; w < 3; ++w) o[w] = res[4 * w] | (res[4 * w + 1] << 8) | (res[4 * w + 2] << 16) | (res[4 * w + 3] << 24);
  }
}

__global__ void __launch_bounds__(256) yolo2d_labels_kernel(const float* __restrict__ rec, int n_rec, const int* __restrict__ lab_i,
                                                          const float* __restrict__ lab_f, int S, int cap, float* __restrict__ cls_o,
                                                          float* __restrict__ box_o, float* __restrict__ bidx_o, int* __restrict__ counts) {
  __shared__ int wsum[4];
  const int b = blockIdx.x;
  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int* ii = lab_i + (size_t)b * YL_I;
  const float* ff = lab_f + (size_t)b * YL_F;
  int total = 0;
  for (int q = 0; q < 8; ++q) total += max(ii[2 * q + 1], 0);
  const int flips = ii[18];
  const float Sf = (float)S, inv = (float)(1.0 / (double)S);
  const size_t row0 = (size_t)b * cap;
  int base = 0;
  for (int c0 = 0; c0 < total; c0 += 256) {
    const int g = c0 + t;
    int k = -1, loc = 0, acc = 0;
    for (int q = 0; q < 8; ++q) {
      const int nq = max(ii[2 * q + 1], 0);
      if (k < 0 && g < acc + nq) {
        k = q;
        loc = g - acc;
      }
      acc += nq;
    }
    bool keep = false;
    float cls = 0.f, bx = 0.f, by = 0.f, bw = 0.f, bh = 0.f;
    const long rrow = k >= 0 ? (long)ii[2 * k] + loc : -1;
    if (k >= 0 && rrow >= 0 && rrow < n_rec) {
      const int layer = k >> 2;
      const int fl = ii[16 + layer];  // bit 0 present, bit 1 mosaic (canvas clip + zero-area filter), bit 2 train (warp + candidates)
      const float* r = rec + (size_t)rrow * 5;
      const float* T = ff + k * 4;
      const float* M = ff + 32 + layer * 8;
      cls = r[0];
      // 1. xywh -> xyxy, x (w, h), + (padw, padh)
      const float dw = r[3] / 2.f, dh = r[4] / 2.f;
      float x1 = r[1] - dw, y1 = r[2] - dh, x2 = r[1] + dw, y2 = r[2] + dh;
      x1 = x1 * T[0]; y1 = y1 * T[1]; x2 = x2 * T[0]; y2 = y2 * T[1];
      x1 = x1 + T[2]; y1 = y1 + T[3]; x2 = x2 + T[2]; y2 = y2 + T[3];
      keep = (fl & 1) != 0;
      if (fl & 2) {
        // 2. clip to the canvas, 3. the zero-area filter
        const float C = 2.f * Sf;
        x1 = fminf(fmaxf(x1, 0.f), C); x2 = fminf(fmaxf(x2, 0.f), C);
        y1 = fminf(fmaxf(y1, 0.f), C); y2 = fminf(fmaxf(y2, 0.f), C);
        keep = keep && ((x2 - x1) * (y2 - y1) > 0.f);
      }
      if (fl & 4) {
        // 4. the four corners through M, min / max
        const float ax = (x1 * M[0] + y1 * M[1]) + M[2], ay = (x1 * M[3] + y1 * M[4]) + M[5];
        const float bx2 = (x2 * M[0] + y2 * M[1]) + M[2], by2 = (x2 * M[3] + y2 * M[4]) + M[5];
        const float cx = (x1 * M[0] + y2 * M[1]) + M[2], cy = (x1 * M[3] + y2 * M[4]) + M[5];
        const float dx = (x2 * M[0] + y1 * M[1]) + M[2], dy = (x2 * M[3] + y1 * M[4]) + M[5];
        float nx1 = fminf(fminf(ax, bx2), fminf(cx, dx)), nx2 = fmaxf(fmaxf(ax, bx2), fmaxf(cx, dx));
        float ny1 = fminf(fminf(ay, by2), fminf(cy, dy)), ny2 = fmaxf(fmaxf(ay, by2), fmaxf(cy, dy));
        // 5. clip to the output
        nx1 = fminf(fmaxf(nx1, 0.f), Sf); nx2 = fminf(fmaxf(nx2, 0.f), Sf);
        ny1 = fminf(fmaxf(ny1, 0.f), Sf); ny2 = fminf(fmaxf(ny2, 0.f), Sf);
        // 6. box_candidates against the pre-warp box x scale
        const float sc = M[6], eps = 1e-16f;
        const float w1 = x2 * sc - x1 * sc, h1 = y2 * sc - y1 * sc;
        const float w2 = nx2 - nx1, h2 = ny2 - ny1;
        const float ar = fmaxf(w2 / (h2 + eps), h2 / (w2 + eps));
        keep = keep && (w2 > 2.f) && (h2 > 2.f) && (w2 * h2 / (w1 * h1 + eps) > 0.1f) && (ar < 100.f);
        x1 = nx1; y1 = ny1; x2 = nx2; y2 = ny2;
      }
      // 7. -> xywh, x 1/S, flips on the normalised centre; the training chain ends in Format's x S, x 1/S
      bx = (x1 + x2) / 2.f; by = (y1 + y2) / 2.f; bw = x2 - x1; bh = y2 - y1;
      bx = bx * inv; by = by * inv; bw = bw * inv; bh = bh * inv;
      if (fl & 4) {
        if (flips & 1) by = 1.f - by;
        if (flips & 2) bx = 1.f - bx;
        bx = bx * Sf; by = by * Sf; bw = bw * Sf; bh = bh * Sf;
        bx = bx * inv; by = by * inv; bw = bw * inv; bh = bh * inv;
      }
    }
    const unsigned long long m = __ballot(keep);
    const int rank = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < 4; ++w) {
      before += w < wave ? wsum[w] : 0;
      all += wsum[w];
    }
    const int row = base + before + rank;
    if (keep && row < cap) {
      const size_t o = row0 + row;
      cls_o[o] = cls;
      *(float4*)(box_o + o * 4) = make_float4(bx, by, bw, bh);
      bidx_o[o] = (float)b;
    }
    base += all;
    __syncthreads();
  }
  for (int j = min(base, cap) + t; j < cap; j += 256) {  // padding rows
    const size_t o = row0 + j;
    cls_o[o] = 0.f;
    *(float4*)(box_o + o * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    bidx_o[o] = -1.f;
  }
  if (t == 0) counts[b] = base;
}

}  // namespace

extern "C" {

int y3d_yolo2d_image_aug(const unsigned char* const* src, int n_src, const int* rec_i, const double* rec_f, const unsigned char* lut, int B,
                         int imgsz, int mode, void* out, void* stream) {
  Y3D_CHECK(src && rec_i && rec_f && lut && out, "yolo2d_image_aug: null argument");
  Y3D_CHECK(B >= 1 && B <= 65535 && n_src >= 1 && (mode == 0 || mode == 1), "yolo2d_image_aug: bad sizes / mode");
  Y3D_CHECK(imgsz >= 4 && imgsz % 4 == 0 && imgsz <= 8192, "yolo2d_image_aug: imgsz %d (a multiple of 4 up to 8192)", imgsz);
  ImgP p{src, n_src, rec_i, rec_f, lut, imgsz, mode};
  hipLaunchKernelGGL(yolo2d_image_kernel, dim3(cdiv((long)imgsz * (imgsz / 4), 256), B), dim3(256), 0, (hipStream_t)stream, p, out);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_yolo2d_encode_labels(const float* rec, int n_rec, const int* lab_i, const float* lab_f, int B, int imgsz, int cap, float* cls,
                             float* bboxes, float* batch_idx, int* counts, void* stream) {
  Y3D_CHECK(rec && lab_i && lab_f && cls && bboxes && batch_idx && counts, "yolo2d_encode_labels: null argument");
  Y3D_CHECK(B >= 1 && n_rec >= 0 && imgsz >= 1, "yolo2d_encode_labels: bad sizes");
  Y3D_CHECK(cap >= 64 && cap <= 512 && cap % 64 == 0, "yolo2d_encode_labels: %d rows per image (64, 128 .. 512)", cap);
  hipLaunchKernelGGL(yolo2d_labels_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, rec, n_rec, lab_i, lab_f, imgsz, cap, cls, bboxes,
                     batch_idx, counts);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

}  // extern "C"
