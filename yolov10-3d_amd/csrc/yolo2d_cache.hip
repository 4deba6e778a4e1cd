// Batch plan over a 2D split that is resident on the device (yolo2d.DeviceSplit): the split's frames live decoded in one arena, with a
// table of pointers to them, their sizes, all label rows and each frame's span of rows in tables indexed by dataset position.  A batch
// is then one small table of random draws; this kernel turns it into the five record arrays y3d_yolo2d_image_aug and
// y3d_yolo2d_encode_labels (yolo2d_batch.hip) take, in their layout, so nothing but the draws crosses PCIe.  Source indices are dataset
// positions (the image kernel gets the split's pointer table, n_src = N) and label rows are counted in the split-wide label table.
//
// A draw row (Y3D_YOLO2D_DRAW_W = 56 float64): two layers of 23 (0: the sample, 1: its MixUp partner)
//   [present, mosaic, warp, frame position of tiles 0..3 (-1: no such tile), yc, xc, canvas side, M 2x3 (float32 values), M_inv (6), scale]
// then at 46: mix, r, hsv, the three gains, flipud, fliplr, bgr, 0.
//
// One workgroup of 256 lanes per sample.  The int / float32 records are assembled in LDS (zeroed, filled by lanes 0..10, copied out by
// one lane per element); rec_f is written by lanes 0..15 and the three HSV tables by lanes 0..191, four entries = one 32-bit word each.
// Everything but the tile geometry and the tables is a copy or a conversion of a value that is float32 already (M, the pads) or a
// float64 -> float32 rounding (scale), as numpy's assignment into a float32 array does it.  Float64 arithmetic, contraction off, in
// this order:
//
//   per tile (lane q = layer * 4 + tile), S = imgsz, (h0, w0) = frame_hw[frame]:
//     r = S / max(h0, w0);  r == 1 -> (h, w) = (h0, w0), else h = min(ceil(h0 * r), S), w = min(ceil(w0 * r), S)      (Split.load)
//     mosaic, integers, C = 2S (Mosaic._mosaic4):
//       tile 0: x1a = max(xc-w, 0), y1a = max(yc-h, 0), x2a = xc, y2a = yc;              x1b = w-(x2a-x1a), y1b = h-(y2a-y1a)
//       tile 1: x1a = xc, y1a = max(yc-h, 0), x2a = min(xc+w, C), y2a = yc;              x1b = 0,           y1b = h-(y2a-y1a)
//       tile 2: x1a = max(xc-w, 0), y1a = yc, x2a = xc, y2a = min(C, yc+h);              x1b = w-(x2a-x1a), y1b = 0
//       tile 3: x1a = xc, y1a = yc, x2a = min(xc+w, C), y2a = min(C, yc+h);              x1b = 0,           y1b = 0
//       padw = x1a - x1b, padh = y1a - y1b; the label pads are (float)padw, (float)padh
//     letter-box (one tile; LetterBox at ratio 1):
//       dw = (S - w) / 2, dh = (S - h) / 2;  left = rint(dw - 0.1), top = rint(dh - 0.1)   (round half to even, as Python's round)
//       x1a = left, y1a = top, x2a = left + w, y2a = top + h, padw = left, padh = top; the label pads are (float)dw, (float)dh
//   HSV tables (RandomHSV), x = 0..255, when the hsv flag is set (zeros otherwise):
//     hue: t = x * g0;  m = fmod(t, 180);  m != 0 and m < 0 -> m + 180   (numpy's float remainder);  (uint8) truncation of m
//     sat / val: t = x * g;  (uint8) truncation of min(max(t, 0), 255)
//
// A frame position outside [0, N) is refused by the entry from the host copy of the draws; the kernel itself skips such a tile (it
// stays all zeros, which the image kernel paints 114 and the label kernel reads as no rows), so a replayed graph whose draws were
// rewritten on the device cannot read outside the tables.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int YC_DRAW = 56;   // == Y3D_YOLO2D_DRAW_W
constexpr int YC_LAYER = 23;  // present, mosaic, warp, frames (4), yc, xc, canvas, M (6), M_inv (6), scale
constexpr int YC_TAIL = 46;   // mix, r, hsv, gains (3), flipud, fliplr, bgr
// the record layouts of yolo2d_batch.hip
constexpr int YI_TILE = 12, YI_LAYER = 50, YI_REC = 112, YI_F = 16, YL_I = 20, YL_F = 48;

static_assert(YC_DRAW == Y3D_YOLO2D_DRAW_W, "the draw row of y3d.h");

struct PlanOut {
  int* rec_i;
  double* rec_f;
  unsigned char* lut;
  int* lab_i;
  float* lab_f;
};

__device__ __forceinline__ unsigned lut_entry(int c, int x, double g) {
  const double t = (double)x * g;
  if (c == 0) {
    double m = fmod(t, 180.0);
    if (m != 0.0 && m < 0.0) m = m + 180.0;
    return (unsigned)(int)m & 255u;
  }
  return (unsigned)(int)fmin(fmax(t, 0.0), 255.0);
}

__global__ void __launch_bounds__(256) yolo2d_plan_kernel(const int* __restrict__ frame_hw, const int* __restrict__ rec_span, int N, int S,
                                                          const double* __restrict__ draws, PlanOut o) {
  __shared__ int s_ri[YI_REC];
  __shared__ int s_li[YL_I];
  __shared__ float s_lf[YL_F];
  const int b = blockIdx.x, t = threadIdx.x;
  const double* d = draws + (size_t)b * YC_DRAW;
  if (t < YI_REC) s_ri[t] = 0;
  if (t < YL_I) s_li[t] = 0;
  if (t < YL_F) s_lf[t] = 0.f;
  __syncthreads();
  if (t < 8) {  // one tile slot
    const int l = t >> 2, k = t & 3;
    const double* L = d + l * YC_LAYER;
    const bool mosaic = L[1] != 0.0;
    const int nt = L[0] != 0.0 ? (mosaic ? 4 : 1) : 0;
    const int f = k < nt ? (int)L[3 + k] : -1;
    if (f >= 0 && f < N) {
      const int h0 = frame_hw[2 * f], w0 = frame_hw[2 * f + 1];
      const double r = (double)S / (double)max(h0, w0);
      int h = h0, w = w0;
      if (r != 1.0) {
        h = min((int)ceil((double)h0 * r), S);
        w = min((int)ceil((double)w0 * r), S);
      }
      int x1a, y1a, x2a, y2a, padw, padh;
      float lpw, lph;
      if (mosaic) {
        const int yc = (int)L[7], xc = (int)L[8], C = 2 * S;
        int x1b, y1b;
        if (k == 0) {
          x1a = max(xc - w, 0); y1a = max(yc - h, 0); x2a = xc; y2a = yc;
          x1b = w - (x2a - x1a); y1b = h - (y2a - y1a);
        } else if (k == 1) {
          x1a = xc; y1a = max(yc - h, 0); x2a = min(xc + w, C); y2a = yc;
          x1b = 0; y1b = h - (y2a - y1a);
        } else if (k == 2) {
          x1a = max(xc - w, 0); y1a = yc; x2a = xc; y2a = min(C, yc + h);
          x1b = w - (x2a - x1a); y1b = 0;
        } else {
          x1a = xc; y1a = yc; x2a = min(xc + w, C); y2a = min(C, yc + h);
          x1b = 0; y1b = 0;
        }
        padw = x1a - x1b;
        padh = y1a - y1b;
        lpw = (float)padw;
        lph = (float)padh;
      } else {
        const double dw = (double)(S - w) / 2.0, dh = (double)(S - h) / 2.0;
        const int top = (int)rint(dh - 0.1), left = (int)rint(dw - 0.1);
        x1a = left; y1a = top; x2a = left + w; y2a = top + h;
        padw = left; padh = top;
        lpw = (float)dw;
        lph = (float)dh;
      }
      int* T = s_ri + l * YI_LAYER + 2 + k * YI_TILE;
      T[0] = f; T[1] = h0; T[2] = w0; T[3] = h; T[4] = w;
      T[5] = x1a; T[6] = y1a; T[7] = x2a; T[8] = y2a; T[9] = padw; T[10] = padh;
      s_li[2 * t] = rec_span[2 * f];
      s_li[2 * t + 1] = rec_span[2 * f + 1];
      s_lf[4 * t] = (float)w;
      s_lf[4 * t + 1] = (float)h;
      s_lf[4 * t + 2] = lpw;
      s_lf[4 * t + 3] = lph;
    }
  } else if (t < 10) {  // one layer's head
    const int l = t - 8;
    const double* L = d + l * YC_LAYER;
    if (L[0] != 0.0) {
      const bool mosaic = L[1] != 0.0;
      s_ri[l * YI_LAYER] = mosaic ? 4 : 1;
      s_ri[l * YI_LAYER + 1] = (int)L[9];
      s_li[16 + l] = 1 | (mosaic ? 2 : 0) | (L[2] != 0.0 ? 4 : 0);
      for (int k = 0; k < 6; ++k) s_lf[32 + l * 8 + k] = (float)L[10 + k];
      s_lf[32 + l * 8 + 6] = (float)L[22];
    }
  } else if (t == 10) {  // the sample's own flags
    const int flipud = d[YC_TAIL + 6] != 0.0 ? 1 : 0, fliplr = d[YC_TAIL + 7] != 0.0 ? 1 : 0;
    s_ri[100] = flipud;
    s_ri[101] = fliplr;
    s_ri[102] = d[YC_TAIL + 8] != 0.0 ? 1 : 0;
    s_ri[103] = d[YC_TAIL + 2] != 0.0 ? 1 : 0;
    s_ri[104] = d[YC_TAIL] != 0.0 ? 1 : 0;
    s_li[18] = flipud | (fliplr << 1);
  }
  __syncthreads();
  if (t < YI_REC) o.rec_i[(size_t)b * YI_REC + t] = s_ri[t];
  if (t < YL_I) o.lab_i[(size_t)b * YL_I + t] = s_li[t];
  if (t < YL_F) o.lab_f[(size_t)b * YL_F + t] = s_lf[t];
  if (t < YI_F) {
    double v = 0.0;
    if (t < 12) {
      const int l = t >= 6 ? 1 : 0;
      const double* L = d + l * YC_LAYER;
      if (L[0] != 0.0) v = L[16 + (t - 6 * l)];
    } else if (t == 12) {
      v = d[YC_TAIL + 1];
    }
    o.rec_f[(size_t)b * YI_F + t] = v;
  }
  if (t < 192) {  // 768 table entries, four to a lane
    unsigned word = 0u;
    if (d[YC_TAIL + 2] != 0.0) {
      const int c = t >> 6, x0 = (t & 63) * 4;
      const double g = d[YC_TAIL + 3 + c];
#pragma unroll
      for (int j = 0; j < 4; ++j) word |= lut_entry(c, x0 + j, g) << (8 * j);
    }
    ((unsigned*)(o.lut + (size_t)b * 768))[t] = word;
  }
}

}  // namespace

extern "C" {

int y3d_yolo2d_plan_batch(const int* frame_hw, const int* rec_span, int N, int imgsz, const double* draws_host, const double* draws, int B,
                          int* rec_i, double* rec_f, unsigned char* lut, int* lab_i, float* lab_f, void* stream) {
  Y3D_CHECK(B >= 1 && N >= 1, "yolo2d_plan_batch: B = %d samples over N = %d frames", B, N);
  Y3D_CHECK(imgsz >= 4 && imgsz % 4 == 0 && imgsz <= 8192, "yolo2d_plan_batch: imgsz %d (a multiple of 4 up to 8192)", imgsz);
  Y3D_CHECK(frame_hw && rec_span && draws_host && draws, "yolo2d_plan_batch: null input");
  Y3D_CHECK(rec_i && rec_f && lut && lab_i && lab_f, "yolo2d_plan_batch: null output");
  Y3D_CHECK(((uintptr_t)lut & 3) == 0, "yolo2d_plan_batch: lut must be 4-byte aligned");
  for (int b = 0; b < B; ++b) {
    const double* d = draws_host + (size_t)b * YC_DRAW;
    Y3D_CHECK(d[0] != 0.0, "yolo2d_plan_batch: sample %d has no primary layer", b);
    for (int l = 0; l < 2; ++l) {
      const double* L = d + l * YC_LAYER;
      if (L[0] == 0.0) continue;
      const int nt = L[1] != 0.0 ? 4 : 1;
      for (int k = 0; k < nt; ++k) {
        const double pos = L[3 + k];
        Y3D_CHECK(pos >= 0.0 && pos < (double)N && pos == (double)(int)pos,
                  "yolo2d_plan_batch: sample %d, layer %d, tile %d: position %g outside [0, %d)", b, l, k, pos, N);
      }
    }
  }
  PlanOut o{rec_i, rec_f, lut, lab_i, lab_f};
  hipLaunchKernelGGL(yolo2d_plan_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, frame_hw, rec_span, N, imgsz, draws, o);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

}  // extern "C"
