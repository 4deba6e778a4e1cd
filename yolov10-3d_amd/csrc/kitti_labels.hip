// Label side of KITTIDataset.__getitem__ (data/datasets/kitti.py:208-405) + collate_fn (:579-599) on the device, in the frame of
// label3d.h: one workgroup per image, one lane per candidate label line, the reference's filter chain per lane, then emit_rows.
//
// Precision follows the reference's numpy arithmetic: boxes and positions are float32 values held in double; mapped box corners,
// centre_2d / size_2d and the whole heading encoding (f32 calibration, python scalars weakly typed) are float32; the projected 3D centre,
// the depth and the size residual are float64.
#include "label3d.h"

namespace {

constexpr int KL_REC = 16;  // packed label record (see y3d.h)

enum { R_CLS = 0, R_TRUNC, R_OCC, R_X1, R_Y1, R_X2, R_Y2, R_H, R_W, R_L, R_PX, R_PY, R_PZ, R_RY };

// DEPTHS: also write the per-line depth table of the foreground depth map (y3d_kitti_depth_map): line_depth[b][wave][lane] = the depth
// label line `lane` of the own (wave 0) or the partner's (wave 1) file paints, the float32 rounding of `zs`, or +inf for a line that is
// dropped or absent.  The filter chain exists once; the flag adds one store per thread.
template <bool DEPTHS>
__global__ void __launch_bounds__(128) kitti_labels_kernel(const double* __restrict__ rec, const int* __restrict__ img_i,
                                                         const double* __restrict__ img_f, int out_w, int out_h, double min_depth,
                                                         double max_depth, int use_camera_dis, const double* __restrict__ mean_size,
                                                         int n_cls, int max_objs, LabelOut o, int* __restrict__ counts,
                                                         double* __restrict__ calib, double* __restrict__ ratio_pad,
                                                         float* __restrict__ line_depth) {
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const ImageRec I(img_i, img_f, b, max_objs);
  bool keep = false;
  float painted = INFINITY;
  Encoded e;
  if (I.live(wave, lane)) {
    const double* r = rec + I.row(wave, lane) * KL_REC;
    e.cls = (int)r[R_CLS];
    const double trunc = r[R_TRUNC], occ = r[R_OCC];
    double x1 = r[R_X1], x2 = r[R_X2];
    const double y1 = r[R_Y1], y2 = r[R_Y2];
    const double h = r[R_H];
    double px = r[R_PX], ry = r[R_RY];
    const double py = r[R_PY], pz = r[R_PZ];
    // difficulty level from the label's own (unflipped) box (kitti_utils.py Object3d.get_obj_level)
    const double height = y2 - y1 + 1.0;
    bool unknown = false;
    if (trunc != -1.0) {
      const bool easy = height >= 40.0 && trunc <= 0.15 && occ <= 0.0;
      const bool moderate = height >= 25.0 && trunc <= 0.3 && occ <= 1.0;
      const bool hard = height >= 25.0 && trunc <= 0.5 && occ <= 2.0;
      unknown = !(easy || moderate || hard);
    }
    if (I.flip) mirror(I, x1, x2, px, ry);
    const double zs = pz * I.scale;
    keep = e.cls >= 0 && e.cls < n_cls;
    keep = keep && !(unknown || zs < min_depth);
    keep = keep && !(trunc > 0.5 || occ > 2.0);
    float X1, X2;
    annotated_box(I, x1, y1, x2, y2, e, X1, X2);
    // 3D centre = pos + (0, -h/2, 0)
    const double cx = px + 0.0, cy = py + (-h / 2.0), cz = pz + 0.0;
    project_centre(I, cx, cy, cz, e);
    keep = keep && centre_inside(e, out_w, out_h);
    keep = keep && !(zs > max_depth);
    if (keep) {
      unit_box(e, (double)e.c2x, (double)e.c2y, (double)e.s2w, (double)e.s2h, out_w, out_h);
      heading_f32(I, ry, ((float)x1 + (float)x2) / 2.f, e);  // at the flipped, untransformed box centre
      size_and_depth(I, mean_size, h, r[R_W], r[R_L], cx, cy, cz, zs, use_camera_dis, e);
      painted = (float)zs;  // never the camera distance (kitti.py:286-287)
    }
  }
  if (DEPTHS) line_depth[((size_t)b * 2 + wave) * 64 + lane] = painted;
  emit_rows(I, b, keep, e, max_objs, out_w, out_h, true, o, counts, calib, ratio_pad);
}

}  // namespace

extern "C" {

int y3d_kitti_encode_labels(const double* rec, const int* img_i, const double* img_f, int B, int out_w, int out_h, double min_depth,
                            double max_depth, int use_camera_dis, const double* mean_size, int n_cls, int max_objs, int64_t* cls,
                            double* bboxes, float* center_2d, float* size_2d, double* center_3d, double* size_3d, double* depth,
                            int64_t* heading_bin, double* heading_res, float* batch_idx, int* counts, double* calib, double* ratio_pad,
                            void* stream) {
  Y3D_CHECK(B >= 1 && img_i && img_f && mean_size && n_cls >= 1, "kitti_encode_labels: bad arguments");
  LabelOut o{cls, bboxes, center_2d, size_2d, center_3d, size_3d, depth, heading_bin, heading_res, batch_idx};
  if (int rc = check_encode_args("kitti_encode_labels", max_objs, out_w, out_h, o, counts, calib, ratio_pad)) return rc;
  hipLaunchKernelGGL(kitti_labels_kernel<false>, dim3(B), dim3(128), 0, (hipStream_t)stream, rec, img_i, img_f, out_w, out_h, min_depth,
                     max_depth, use_camera_dis, mean_size, n_cls, max_objs, o, counts, calib, ratio_pad, (float*)nullptr);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_kitti_encode_labels_depths(const double* rec, const int* img_i, const double* img_f, int B, int out_w, int out_h, double min_depth,
                                   double max_depth, int use_camera_dis, const double* mean_size, int n_cls, int max_objs, int64_t* cls,
                                   double* bboxes, float* center_2d, float* size_2d, double* center_3d, double* size_3d, double* depth,
                                   int64_t* heading_bin, double* heading_res, float* batch_idx, int* counts, double* calib,
                                   double* ratio_pad, float* line_depth, void* stream) {
  Y3D_CHECK(B >= 1 && img_i && img_f && mean_size && n_cls >= 1 && line_depth, "kitti_encode_labels_depths: bad arguments");
  LabelOut o{cls, bboxes, center_2d, size_2d, center_3d, size_3d, depth, heading_bin, heading_res, batch_idx};
  if (int rc = check_encode_args("kitti_encode_labels_depths", max_objs, out_w, out_h, o, counts, calib, ratio_pad)) return rc;
  hipLaunchKernelGGL(kitti_labels_kernel<true>, dim3(B), dim3(128), 0, (hipStream_t)stream, rec, img_i, img_f, out_w, out_h, min_depth,
                     max_depth, use_camera_dis, mean_size, n_cls, max_objs, o, counts, calib, ratio_pad, line_depth);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

}  // extern "C"
