// Batch plan over a KITTI split that is resident on the device (kitti.DeviceSplit): the split's frames live decoded in one arena with
// their label records, spans, sizes and both calibrations (as read, and mirrored) in tables indexed by dataset position.  A batch is
// then one small table of random draws; this kernel turns it into the per-image tables y3d_kitti_image_aug (post.hip) and
// y3d_kitti_encode_labels (kitti_labels.hip) take, so nothing but the draws crosses PCIe.  One thread per image, copies only: the only
// arithmetic is the float32 -> float64 widening of the calibration, which is exact.
#include "common.h"

namespace {

constexpr int KC_DRAW = 16;  // pos, partner (-1: none), flip, scale, trans (6), trans_inv (6)
constexpr int KC_IMGF = 19;  // as kitti_labels.hip: P2 (12), trans (6), scale
constexpr int KC_IMGI = 7;   // as kitti_labels.hip: primary start, lines, partner start, lines, flip, width, height

struct PlanOut {
  const unsigned char** src;
  const unsigned char** src2;
  int* hw;
  int* flip;
  double* trans_inv;
  int* img_i;
  double* img_f;
  unsigned char* mixed;
};

__global__ void __launch_bounds__(64) kitti_plan_kernel(const int64_t* __restrict__ img_off, const int* __restrict__ frame_hw,
                                                        const int* __restrict__ rec_span, const float* __restrict__ P2,
                                                        const unsigned char* arena, const double* __restrict__ draws, int B, PlanOut o) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* d = draws + (size_t)b * KC_DRAW;
  const int pos = (int)d[0], par = (int)d[1];  // both checked against the table on the host
  const int fl = d[2] != 0.0 ? 1 : 0;
  const int H = frame_hw[pos * 2], W = frame_hw[pos * 2 + 1];
  o.src[b] = arena + img_off[pos];
  o.src2[b] = par >= 0 ? arena + img_off[par] : nullptr;
  o.hw[b * 2] = H;
  o.hw[b * 2 + 1] = W;
  o.flip[b] = fl;
  o.mixed[b] = par >= 0 ? 1 : 0;
  for (int k = 0; k < 6; ++k) o.trans_inv[b * 6 + k] = d[10 + k];
  int* ii = o.img_i + (size_t)b * KC_IMGI;
  const int row0 = rec_span[pos * 2], n0 = rec_span[pos * 2 + 1];
  ii[0] = row0;
  ii[1] = n0;
  ii[2] = par >= 0 ? rec_span[par * 2] : row0 + n0;
  ii[3] = par >= 0 ? rec_span[par * 2 + 1] : 0;
  ii[4] = fl;
  ii[5] = W;
  ii[6] = H;
  double* f = o.img_f + (size_t)b * KC_IMGF;
  const float* P = P2 + ((size_t)pos * 2 + fl) * 12;
  for (int k = 0; k < 12; ++k) f[k] = (double)P[k];
  for (int k = 0; k < 6; ++k) f[12 + k] = d[4 + k];
  f[18] = d[3];
}

}  // namespace

extern "C" {

int y3d_kitti_plan_batch(const int64_t* img_off, const int* frame_hw, const int* rec_span, const float* P2, int N,
                         const unsigned char* arena, const double* draws_host, const double* draws, int B, const unsigned char** src,
                         const unsigned char** src2, int* hw, int* flip, double* trans_inv, int* img_i, double* img_f,
                         unsigned char* mixed, void* stream) {
  Y3D_CHECK(B >= 1 && N >= 1, "kitti_plan_batch: B = %d images over N = %d frames", B, N);
  Y3D_CHECK(img_off && frame_hw && rec_span && P2 && arena && draws_host && draws, "kitti_plan_batch: null input");
  Y3D_CHECK(src && src2 && hw && flip && trans_inv && img_i && img_f && mixed, "kitti_plan_batch: null output");
  for (int b = 0; b < B; ++b) {
    const double pos = draws_host[(size_t)b * KC_DRAW], par = draws_host[(size_t)b * KC_DRAW + 1];
    Y3D_CHECK(pos >= 0.0 && pos < (double)N && pos == (double)(int)pos, "kitti_plan_batch: image %d: position %g outside [0, %d)", b, pos, N);
    Y3D_CHECK(par == -1.0 || (par >= 0.0 && par < (double)N && par == (double)(int)par),
              "kitti_plan_batch: image %d: partner %g is neither -1 nor in [0, %d)", b, par, N);
  }
  PlanOut o{src, src2, hw, flip, trans_inv, img_i, img_f, mixed};
  hipLaunchKernelGGL(kitti_plan_kernel, dim3(cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, img_off, frame_hw, rec_span, P2, arena, draws, B,
                     o);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

}  // extern "C"
