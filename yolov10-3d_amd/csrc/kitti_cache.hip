// Batch plan over a KITTI split that is resident on the device (kitti.DeviceSplit): the split's frames live decoded in one arena with
// their label records, spans, sizes and both calibrations (as read, and mirrored; float32) in tables indexed by dataset position.  A
// batch is one small table of random draws; plan3d_kernel (label3d.h) turns it into the per-image tables y3d_kitti_image_aug (post.hip)
// and y3d_kitti_encode_labels (kitti_labels.hip) take.
#include "label3d.h"

extern "C" {

int y3d_kitti_plan_batch(const int64_t* img_off, const int* frame_hw, const int* rec_span, const float* P2, int N,
                         const unsigned char* arena, const double* draws_host, const double* draws, int B, const unsigned char** src,
                         const unsigned char** src2, int* hw, int* flip, double* trans_inv, int* img_i, double* img_f,
                         unsigned char* mixed, void* stream) {
  Y3D_CHECK(B >= 1 && N >= 1, "kitti_plan_batch: B = %d images over N = %d frames", B, N);
  Y3D_CHECK(img_off && frame_hw && rec_span && P2 && arena && draws_host && draws, "kitti_plan_batch: null input");
  Y3D_CHECK(src && src2 && hw && flip && trans_inv && img_i && img_f && mixed, "kitti_plan_batch: null output");
  if (int rc = check_draw_positions("kitti_plan_batch", draws_host, B, L3_DRAW, N)) return rc;
  PlanOut o{src, src2, hw, flip, trans_inv, img_i, img_f, mixed};
  hipLaunchKernelGGL((plan3d_kernel<float, false>), dim3(cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, img_off, frame_hw, rec_span, P2, arena,
                     (const unsigned char*)nullptr, draws, B, o);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

}  // extern "C"
