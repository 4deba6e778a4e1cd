// Batch plan over a Waymo / Omni3D split that is resident in two tiers (json3d.DeviceSplit): the first n_dev frames of the split live
// decoded in a device arena, the rest in pinned host memory, from where the frames a batch uses are copied into a per-batch staging
// buffer before this kernel runs.  The label records, spans, sizes and both calibrations (the float64 one as read, and the float32 one
// of the mirrored image, widened) are in device tables indexed by dataset position.  A batch is one small table of random draws; this
// kernel turns it into the per-image tables y3d_kitti_image_aug (post.hip) and y3d_json3d_encode_labels (json3d_labels.hip) take.
// One thread per image, copies only.  A frame's source is the staging buffer when its row names a staging offset, the arena
// otherwise: img_off holds -1 at the positions of the host tier and is never read for them.
#include "common.h"

namespace {

constexpr int JC_DRAW = Y3D_JSON3D_DRAW_W;  // pos, partner (-1: none), flip, scale, trans (6), trans_inv (6), staging offset of both (-1: arena)
constexpr int JC_IMGF = 19;                 // as json3d_labels.hip: P2 (12), trans (6), scale
constexpr int JC_IMGI = 7;                  // as json3d_labels.hip: primary start, objects, partner start, objects, flip, width, height

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

__global__ void __launch_bounds__(64) json3d_plan_kernel(const int64_t* __restrict__ img_off, const int* __restrict__ frame_hw,
                                                         const int* __restrict__ rec_span, const double* __restrict__ P2,
                                                         const unsigned char* arena, const unsigned char* stage,
                                                         const double* __restrict__ draws, int B, PlanOut o) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* d = draws + (size_t)b * JC_DRAW;
  const int pos = (int)d[0], par = (int)d[1];  // both, and the two staging offsets, checked against the table on the host
  const int fl = d[2] != 0.0 ? 1 : 0;
  const int H = frame_hw[pos * 2], W = frame_hw[pos * 2 + 1];
  const unsigned char* s0 = d[16] >= 0.0 ? stage + (int64_t)d[16] : arena + img_off[pos];
  const unsigned char* s1 = nullptr;
  if (par >= 0) s1 = d[17] >= 0.0 ? stage + (int64_t)d[17] : arena + img_off[par];
  o.src[b] = s0;
  o.src2[b] = s1;
  o.hw[b * 2] = H;
  o.hw[b * 2 + 1] = W;
  o.flip[b] = fl;
  o.mixed[b] = par >= 0 ? 1 : 0;
  for (int k = 0; k < 6; ++k) o.trans_inv[b * 6 + k] = d[10 + k];
  int* ii = o.img_i + (size_t)b * JC_IMGI;
  const int row0 = rec_span[pos * 2], n0 = rec_span[pos * 2 + 1];
  ii[0] = row0;
  ii[1] = n0;
  ii[2] = par >= 0 ? rec_span[par * 2] : row0 + n0;
  ii[3] = par >= 0 ? rec_span[par * 2 + 1] : 0;
  ii[4] = fl;
  ii[5] = W;
  ii[6] = H;
  double* f = o.img_f + (size_t)b * JC_IMGF;
  const double* P = P2 + ((size_t)pos * 2 + fl) * 12;
  for (int k = 0; k < 12; ++k) f[k] = P[k];
  for (int k = 0; k < 6; ++k) f[12 + k] = d[4 + k];
  f[18] = d[3];
}

// 0 when the staging offset `so` of the frame at position `pos` is what its tier asks for, else the number of the rule it breaks
int stage_fault(double pos, double so, int n_dev, int64_t stage_bytes) {
  if (pos < (double)n_dev) return so == -1.0 ? 0 : 1;  // resident in the arena: no offset
  if (so == -1.0) return 2;                            // host tier: staged, or the kernel would read img_off's -1
  if (!(so >= 0.0) || so != (double)(int64_t)so || ((int64_t)so & 15) != 0) return 3;
  return so < (double)stage_bytes ? 0 : 4;
}

const char* const kStageFault[] = {"", "has a staging offset but is resident in the arena", "lies in the host tier and has no staging offset",
                                   "has a staging offset that is no multiple of 16 from 0 up", "has a staging offset outside the staging buffer"};

}  // namespace

extern "C" {

int y3d_json3d_plan_batch(const int64_t* img_off, const int* frame_hw, const int* rec_span, const double* P2, int N, int n_dev,
                          const unsigned char* arena, const unsigned char* stage, int64_t stage_bytes, const double* draws_host,
                          const double* draws, int B, const unsigned char** src, const unsigned char** src2, int* hw, int* flip,
                          double* trans_inv, int* img_i, double* img_f, unsigned char* mixed, void* stream) {
  Y3D_CHECK(B >= 1 && N >= 1, "json3d_plan_batch: B = %d images over N = %d frames", B, N);
  Y3D_CHECK(n_dev >= 0 && n_dev <= N && stage_bytes >= 0, "json3d_plan_batch: n_dev = %d of N = %d frames, a staging buffer of %lld bytes",
            n_dev, N, (long long)stage_bytes);
  Y3D_CHECK(img_off && frame_hw && rec_span && P2 && draws_host && draws, "json3d_plan_batch: null input");
  Y3D_CHECK(arena || n_dev == 0, "json3d_plan_batch: null arena for %d resident frames", n_dev);
  Y3D_CHECK(src && src2 && hw && flip && trans_inv && img_i && img_f && mixed, "json3d_plan_batch: null output");
  for (int b = 0; b < B; ++b) {
    const double* d = draws_host + (size_t)b * JC_DRAW;
    const double pos = d[0], par = d[1];
    Y3D_CHECK(pos >= 0.0 && pos < (double)N && pos == (double)(int)pos, "json3d_plan_batch: image %d: position %g outside [0, %d)", b, pos, N);
    Y3D_CHECK(par == -1.0 || (par >= 0.0 && par < (double)N && par == (double)(int)par),
              "json3d_plan_batch: image %d: partner %g is neither -1 nor in [0, %d)", b, par, N);
    int fault = stage_fault(pos, d[16], n_dev, stage_bytes);
    Y3D_CHECK(fault == 0, "json3d_plan_batch: image %d: position %g %s (offset %g, n_dev %d, %lld bytes)", b, pos, kStageFault[fault], d[16],
              n_dev, (long long)stage_bytes);
    if (par >= 0.0) {
      fault = stage_fault(par, d[17], n_dev, stage_bytes);
      Y3D_CHECK(fault == 0, "json3d_plan_batch: image %d: partner %g %s (offset %g, n_dev %d, %lld bytes)", b, par, kStageFault[fault], d[17],
                n_dev, (long long)stage_bytes);
    } else {
      Y3D_CHECK(d[17] == -1.0, "json3d_plan_batch: image %d: a staging offset %g without a partner", b, d[17]);
    }
    Y3D_CHECK(stage || (d[16] < 0.0 && d[17] < 0.0), "json3d_plan_batch: image %d: a staging offset but a null staging buffer", b);
  }
  PlanOut o{src, src2, hw, flip, trans_inv, img_i, img_f, mixed};
  hipLaunchKernelGGL(json3d_plan_kernel, dim3(cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, img_off, frame_hw, rec_span, P2, arena, stage,
                     draws, B, o);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

}  // extern "C"
