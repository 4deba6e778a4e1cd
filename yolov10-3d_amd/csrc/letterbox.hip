// Rectangular letter-boxing on the device, for the two callers that hand the 2D models images that are not square training canvases:
// the validator's rect=True batches (data/base.py set_rectangle :226-249, load_image :147-182; data/augment.py LetterBox :684-750,
// Format :915-957; collate_fn data/dataset.py:206-223) and the predictor (engine/predictor.py preprocess / pre_transform :115-156,
// models/yolov10/predict.py:8-38, utils/ops.py scale_boxes / clip_boxes :89-124, :127-145).  Host code (yolo2d.py, predict.py) replays
// the reference's shape, pad and rounding arithmetic; three kernels do the rest.
//
// y3d_letterbox_image — one launch per batch, one thread per FOUR neighbouring output pixels of a row of the (H, W) canvas.  The image
// index is blockIdx.y, so the eight ints of the record [src, h0, w0, new_h, new_w, top, left, swap_rb] are uniform loads.  Per pixel:
//
//   outside [top, top + new_h) x [left, left + new_w)  ->  114, nothing is read
//   ty = oy - top, tx = ox - left
//   (new_h, new_w) == (h0, w0)                         ->  the source pixel (ty, tx) itself, no floating-point work
//   else, float64 with contraction off, + - * / and floor only (the tile arithmetic of yolo2d_batch.hip, tests/yolo2d_ref.py resize):
//        fx = (tx + 0.5)*(w0/new_w) - 0.5,  X0 = floor(fx), bx = fx - X0;  X0 < 0 -> (0, bx 0);  X0 >= w0-1 -> (w0-1, bx 0);  same in y
//        v = ((p00*(1-bx) + p01*bx)*(1-by)) + ((p10*(1-bx) + p11*bx)*by);   pixel = floor(v + 0.5)
//      the row's y taps are computed once per thread; a tap whose weight is exactly zero is not loaded (its product is an exact zero).
//   swap_rb exchanges channels 0 and 2 (the predictor's BGR -> RGB).
//   mode 0: (B, 3, H, W) float32 = value / 255, one float4 per plane; mode 1: (B, H, W, 3) uint8, the thread's 12 bytes as three words.
//
// One resize stage covers both callers: a rect validation sample is load_image's resize (long side -> imgsz) followed by a letter-box of
// ratio 1, the predictor's is one resize from the original.  The records are trusted once the host has checked them (yolo2d.pack_letterbox);
// a record whose source index is out of range or whose sizes are below 1 is not read and gives an all-114 image, it raises nothing.
// This is not OpenCV's fixed-point resize.
//
// y3d_letterbox_labels — LetterBox._update_labels + Format for a validation sample, float32 in the reference's order, one workgroup per
// image, one label row per lane: xywh -> xyxy, x (w, h), + (padw, padh) (the fractional dw, dh), -> xywh, x (1/W, 1/H).  Nothing is
// filtered, so file order is output order.
//
// y3d_predict_rows — the predictor's confidence / class filter and scale_boxes + clip_boxes, one workgroup per image; the rows are walked
// in chunks of 256 and the survivors compacted in their (score) order: ballot + popcount within a wave, an LDS prefix over the four
// waves, a running base across chunks.  float32 with IEEE division: (x - pad) / gain, as torch's in-place `-= pad; /= gain` computes it.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int LB_REC = 8;  // src, h0, w0, new_h, new_w, top, left, swap_rb

struct Tap {
  int i0, i1;
  double b;
};

// the two taps and the weight of output coordinate t on an axis resized n0 -> n
__device__ __forceinline__ Tap axis_tap(int t, int n, int n0) {
  const double f = ((double)t + 0.5) * ((double)n0 / (double)n) - 0.5;
  const double ff = floor(f);
  Tap a;
  a.b = f - ff;
  a.i0 = (int)ff;
  if (a.i0 < 0) { a.i0 = 0; a.b = 0.0; }
  if (a.i0 >= n0 - 1) { a.i0 = n0 - 1; a.b = 0.0; }
  a.i1 = min(a.i0 + 1, n0 - 1);
  return a;
}

__global__ void __launch_bounds__(256) letterbox_image_kernel(const unsigned char* const* __restrict__ src, int n_src,
                                                            const int* __restrict__ rec, int H, int W, int mode, void* __restrict__ out) {
  const int b = blockIdx.y;
  const int groups = W >> 2;  // W % 4 == 0 (checked by the entry)
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= H * groups) return;
  const int oy = g / groups, ox4 = (g - oy * groups) * 4;
  const int* R = rec + (size_t)b * LB_REC;
  const int s = R[0], h0 = R[1], w0 = R[2], nh = R[3], nw = R[4], top = R[5], left = R[6], swap = R[7];
  const bool ok = s >= 0 && s < n_src && h0 >= 1 && w0 >= 1 && nh >= 1 && nw >= 1;
  const int ty = oy - top;
  const bool row_in = ok && ty >= 0 && ty < nh;
  const bool copy = nh == h0 && nw == w0;
  unsigned res[12];  // four pixels x three channels, in the output's channel order
#pragma unroll
  for (int k = 0; k < 12; ++k) res[k] = 114u;
  if (row_in) {
    const unsigned char* p = src[s];
    Tap ya;
    ya.i0 = ya.i1 = ty;
    ya.b = 0.0;
    if (!copy) ya = axis_tap(ty, nh, h0);
    const unsigned char* r0 = p + (size_t)ya.i0 * w0 * 3;
    const unsigned char* r1 = p + (size_t)ya.i1 * w0 * 3;
    const double by = ya.b;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int tx = ox4 + j - left;
      if (tx < 0 || tx >= nw) continue;
      unsigned v[3];
      if (copy) {
        const unsigned char* q = r0 + (size_t)tx * 3;
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
      } else {
        const Tap xa = axis_tap(tx, nw, w0);
        const double bx = xa.b;
        const unsigned char* q00 = r0 + (size_t)xa.i0 * 3;
        const unsigned char* q01 = r0 + (size_t)xa.i1 * 3;
        const unsigned char* q10 = r1 + (size_t)xa.i0 * 3;
        const unsigned char* q11 = r1 + (size_t)xa.i1 * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double p00 = (double)q00[c];
          const double p01 = bx != 0.0 ? (double)q01[c] : 0.0;
          const double p10 = by != 0.0 ? (double)q10[c] : 0.0;
          const double p11 = (by != 0.0 && bx != 0.0) ? (double)q11[c] : 0.0;
          const double w = ((p00 * (1.0 - bx) + p01 * bx) * (1.0 - by)) + ((p10 * (1.0 - bx) + p11 * bx) * by);
          v[c] = (unsigned)fmin(fmax(floor(w + 0.5), 0.0), 255.0);
        }
      }
      res[j * 3 + 0] = swap ? v[2] : v[0];
      res[j * 3 + 1] = v[1];
      res[j * 3 + 2] = swap ? v[0] : v[2];
    }
  }
  if (mode == 0) {
    float* o = (float*)out;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float4 q = make_float4((float)res[c] / 255.f, (float)res[3 + c] / 255.f, (float)res[6 + c] / 255.f, (float)res[9 + c] / 255.f);
      *(float4*)(o + (((size_t)b * 3 + c) * H + oy) * W + ox4) = q;
    }
  } else {
    unsigned* o = (unsigned*)((unsigned char*)out + (((size_t)b * H + oy) * W + ox4) * 3);
#pragma unroll
    for (int w = 0; w < 3; ++w) o[w] = res[4 * w] | (res[4 * w + 1] << 8) | (res[4 * w + 2] << 16) | (res[4 * w + 3] << 24);
  }
}

__global__ void __launch_bounds__(256) letterbox_labels_kernel(const float* __restrict__ rec, int n_rec, const int* __restrict__ lab_i,
                                                             const float* __restrict__ lab_f, int H, int W, int cap,
                                                             float* __restrict__ cls_o, float* __restrict__ box_o,
                                                             float* __restrict__ bidx_o, int* __restrict__ counts) {
  const int b = blockIdx.x;
  const int t = threadIdx.x;
  const int first = lab_i[2 * b];
  int n = lab_i[2 * b + 1];
  if (first < 0 || n < 0 || (long)first + n > n_rec) n = 0;  // rows outside the table are not read
  const float iw = lab_f[4 * b], ih = lab_f[4 * b + 1], padw = lab_f[4 * b + 2], padh = lab_f[4 * b + 3];
  const float invw = (float)(1.0 / (double)W), invh = (float)(1.0 / (double)H);
  const size_t row0 = (size_t)b * cap;
  const int used = min(n, cap);
  for (int j = t; j < cap; j += 256) {
    const size_t o = row0 + j;
    if (j < used) {
      const float* r = rec + ((size_t)first + j) * 5;
      const float dw = r[3] / 2.f, dh = r[4] / 2.f;
      float x1 = r[1] - dw, y1 = r[2] - dh, x2 = r[1] + dw, y2 = r[2] + dh;
      x1 = x1 * iw; y1 = y1 * ih; x2 = x2 * iw; y2 = y2 * ih;
      x1 = x1 + padw; y1 = y1 + padh; x2 = x2 + padw; y2 = y2 + padh;
      float bx = (x1 + x2) / 2.f, by = (y1 + y2) / 2.f, bw = x2 - x1, bh = y2 - y1;
      bx = bx * invw; by = by * invh; bw = bw * invw; bh = bh * invh;
      cls_o[o] = r[0];
      *(float4*)(box_o + o * 4) = make_float4(bx, by, bw, bh);
      bidx_o[o] = (float)b;
    } else {  // padding rows
      cls_o[o] = 0.f;
      *(float4*)(box_o + o * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
      bidx_o[o] = -1.f;
    }
  }
  if (t == 0) counts[b] = n;
}

__global__ void __launch_bounds__(256) predict_rows_kernel(const float* __restrict__ preds, const float* __restrict__ meta, float conf,
                                                         const int* __restrict__ classes, int n_cls, int K, float* __restrict__ out,
                                                         int* __restrict__ counts) {
  __shared__ int wsum[4];
  const int b = blockIdx.x;
  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const float* M = meta + (size_t)b * 5;
  const float h0 = M[0], w0 = M[1], gain = M[2], padw = M[3], padh = M[4];
  const float2* in = (const float2*)(preds + (size_t)b * K * 6);  // rows of 24 bytes: 8-byte aligned
  float2* o = (float2*)(out + (size_t)b * K * 6);
  int base = 0;
  for (int c0 = 0; c0 < K; c0 += 256) {
    const int k = c0 + t;
    bool keep = false;
    float2 a = make_float2(0.f, 0.f), c = a, d = a;
    if (k < K) {
      a = in[(size_t)k * 3];
      c = in[(size_t)k * 3 + 1];
      d = in[(size_t)k * 3 + 2];
      keep = d.x > conf;
      if (n_cls > 0) {
        bool hit = false;
        for (int i = 0; i < n_cls; ++i) hit = hit || (d.y == (float)classes[i]);
        keep = keep && hit;
      }
      a.x = fminf(fmaxf((a.x - padw) / gain, 0.f), w0);
      a.y = fminf(fmaxf((a.y - padh) / gain, 0.f), h0);
      c.x = fminf(fmaxf((c.x - padw) / gain, 0.f), w0);
      c.y = fminf(fmaxf((c.y - padh) / gain, 0.f), h0);
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
    if (keep) {  // base + before + rank <= k < K
      const size_t r = (size_t)(base + before + rank) * 3;
      o[r] = a;
      o[r + 1] = c;
      o[r + 2] = d;
    }
    base += all;
    __syncthreads();
  }
  // the rows behind the survivors: a survivor is never written past its own input row, and every input row was loaded before the
  // chunk's barrier, so in-place use is not supported but out != preds never races
  for (int j = base + t; j < K; j += 256) {
    const float2 z = make_float2(0.f, 0.f);
    o[(size_t)j * 3] = z;
    o[(size_t)j * 3 + 1] = z;
    o[(size_t)j * 3 + 2] = z;
  }
  if (t == 0) counts[b] = base;
}

}  // namespace

extern "C" {

int y3d_letterbox_image(const unsigned char* const* src_table, int n_src, const int* rec, int B, int H, int W, int mode, void* out,
                        void* stream) {
  Y3D_CHECK(src_table && rec && out, "letterbox_image: null argument");
  Y3D_CHECK(B >= 1 && B <= 65535 && n_src >= 1 && (mode == 0 || mode == 1), "letterbox_image: bad sizes / mode");
  Y3D_CHECK(H >= 1 && H <= 8192 && W >= 4 && W <= 8192 && W % 4 == 0, "letterbox_image: canvas %d x %d (W a multiple of 4, both up to 8192)", H, W);
  hipLaunchKernelGGL(letterbox_image_kernel, dim3(cdiv((long)H * (W / 4), 256), B), dim3(256), 0, (hipStream_t)stream, src_table, n_src, rec,
                     H, W, mode, out);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_letterbox_labels(const float* rec, int n_rec, const int* lab_i, const float* lab_f, int B, int H, int W, int cap, float* cls,
                         float* bboxes, float* batch_idx, int* counts, void* stream) {
  Y3D_CHECK(rec && lab_i && lab_f && cls && bboxes && batch_idx && counts, "letterbox_labels: null argument");
  Y3D_CHECK(B >= 1 && n_rec >= 0 && H >= 1 && W >= 1, "letterbox_labels: bad sizes");
  Y3D_CHECK(cap >= 64 && cap <= 512 && cap % 64 == 0, "letterbox_labels: %d rows per image (64, 128 .. 512)", cap);
  hipLaunchKernelGGL(letterbox_labels_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, rec, n_rec, lab_i, lab_f, H, W, cap, cls, bboxes,
                     batch_idx, counts);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_predict_rows(const float* preds, const float* meta, float conf, const int* classes, int n_cls, int B, int K, float* out, int* counts,
                     void* stream) {
  Y3D_CHECK(preds && meta && out && counts, "predict_rows: null argument");
  Y3D_CHECK(out != preds, "predict_rows: in-place use is not supported");
  Y3D_CHECK(B >= 1 && K >= 1 && n_cls >= 0 && (n_cls == 0 || classes), "predict_rows: bad sizes");
  hipLaunchKernelGGL(predict_rows_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, preds, meta, conf, classes, n_cls, K, out, counts);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

}  // extern "C"
