// Batch plan over a Waymo / Omni3D split that is resident in two tiers (json3d.DeviceSplit): the first n_dev frames of the split live
// decoded in a device arena, the rest in pinned host memory, from where the frames a batch uses are copied into a per-batch staging
// buffer before this kernel runs.  The label records, spans, sizes and both calibrations (the float64 one as read, and the float32 one
// of the mirrored image, widened) are in device tables indexed by dataset position.  A batch is one small table of random draws;
// plan3d_kernel (label3d.h) turns it into the per-image tables y3d_kitti_image_aug (post.hip) and y3d_json3d_encode_labels
// (json3d_labels.hip) take.  A frame's source is the staging buffer when its row names a staging offset, the arena otherwise:
// img_off holds -1 at the positions of the host tier and is never read for them.
#include "label3d.h"

namespace {

static_assert(Y3D_JSON3D_DRAW_W == L3_DRAW + 2, "the draw table: the shared columns, then the staging offset of the primary and of the partner");

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
  if (int rc = check_draw_positions("json3d_plan_batch", draws_host, B, Y3D_JSON3D_DRAW_W, N)) return rc;
  for (int b = 0; b < B; ++b) {
    const double* d = draws_host + (size_t)b * Y3D_JSON3D_DRAW_W;
    const double pos = d[0], par = d[1];
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
  hipLaunchKernelGGL((plan3d_kernel<double, true>), dim3(cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, img_off, frame_hw, rec_span, P2, arena,
                     stage, draws, B, o);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

}  // extern "C"
