// Label side of WaymoDataset.__getitem__ (data/datasets/waymo.py:186-290, load_object :292-372) and Omni3Dataset.__getitem__
// (data/datasets/omni3d.py:175-279, load_object :281-352) + their collate_fn on the device, in the frame of label3d.h: one workgroup
// per image, one lane per candidate object, the dataset's filter chain per lane, then emit_rows.
//
// Precision follows the reference operation by operation.  Positions, dimensions and ry are float64 (they come from JSON); the
// annotated box is float32.  The calibration is float64 as read and float32 once mirrored (Calibration.flip), so tx / ty and the
// heading's arctan2 are float32 exactly when the image is mirrored.  Waymo's box is recomputed from the eight corners that
// keypoint_utils.get_object_keypoints builds in float32 (rotation from float32 sin / cos, corners cast to float32, three-term sums
// accumulated in j order) and adds to the float64 centre; every point is cast to float32 before it goes through the crop matrix.
#include "label3d.h"

namespace {

constexpr int JL_REC = 24;  // packed object record (see y3d.h)

enum { R_CLS = 0, R_X1, R_Y1, R_X2, R_Y2, R_H, R_W, R_L, R_PX, R_PY, R_PZ, R_RY, R_LIDAR, R_BEHIND, R_VALID, R_DERR, R_TRUNC, R_VIS };

// Waymo's recompute_bbox_2d: the corners of get_object_keypoints(centre, (h, w, l), ry), rotation Rx(pi/2) Ry(-ry) Rz(0) in float32,
// projected in float64; their extremes cast to float32 go through the crop map in float64 -> the box as xywh; centre_2d / size_2d
__device__ __forceinline__ void corner_box(const ImageRec& I, double h, double w, double l, double ry, double cx, double cy, double cz,
                                           Encoded& e, double& bcx, double& bcy, double& bw, double& bh) {
  const float ang = -(float)ry;
  const float ca = (float)cos((double)ang), sa = (float)sin((double)ang);
  const float cq = -4.37113883e-08f;  // cos(float32(pi / 2)); its sine is 1
  const float m20 = cq * -sa, m22 = cq * ca;
  const float hl = (float)(l / 2.0), hw = (float)(w / 2.0), hh = (float)(h / 2.0);
  double umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float bx = (k & 2) ? -hl : hl, by = (k & 1) ? -hw : hw, bz = (k & 4) ? hh : -hh;
    const float X = ((0.f + ca * bx) + sa * by) + m20 * bz;
    const float Y = ((0.f + 0.f * bx) + cq * by) + 1.f * bz;
    const float Z = ((0.f + sa * bx) + -ca * by) + m22 * bz;
    const double kx = (double)X + cx, ky = (double)Y + cy, kz = (double)Z + cz;
    const double ku = (kx * I.p00 + ky * I.p01 + kz * I.p02 + I.p03) / kz;
    const double kv = (kx * I.p10 + ky * I.p11 + kz * I.p12 + I.p13) / kz;
    umin = fmin(umin, ku);
    umax = fmax(umax, ku);
    vmin = fmin(vmin, kv);
    vmax = fmax(vmax, kv);
  }
  const double a0 = (double)(float)umin, a1 = (double)(float)vmin, a2 = (double)(float)umax, a3 = (double)(float)vmax;
  const double X1 = I.t00 * a0 + I.t01 * a1 + I.t02, Y1 = I.t10 * a0 + I.t11 * a1 + I.t12;
  const double X2 = I.t00 * a2 + I.t01 * a3 + I.t02, Y2 = I.t10 * a2 + I.t11 * a3 + I.t12;
  bcx = (X1 + X2) / 2.0;
  bcy = (Y1 + Y2) / 2.0;
  bw = X2 - X1;
  bh = Y2 - Y1;
  e.c2x = (float)bcx;
  e.c2y = (float)bcy;
  e.s2w = (float)bw;
  e.s2h = (float)bh;
}

__global__ void __launch_bounds__(128) json3d_labels_kernel(const double* __restrict__ rec, const int* __restrict__ img_i,
                                                          const double* __restrict__ img_f, int dataset, int out_w, int out_h,
                                                          double min_depth, double max_depth, int use_camera_dis,
                                                          const double* __restrict__ mean_size, int n_cls, int max_objs, LabelOut o,
                                                          int* __restrict__ counts, double* __restrict__ calib,
                                                          double* __restrict__ ratio_pad) {
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const ImageRec I(img_i, img_f, b, max_objs);
  bool keep = false;
  Encoded e;
  if (I.live(wave, lane)) {
    const double* r = rec + I.row(wave, lane) * JL_REC;
    e.cls = (int)r[R_CLS];
    double x1 = r[R_X1], x2 = r[R_X2];
    const double y1 = r[R_Y1], y2 = r[R_Y2];
    const double h = r[R_H], w = r[R_W], l = r[R_L];
    double px = r[R_PX], ry = r[R_RY];
    const double py = r[R_PY], pz = r[R_PZ];
    if (I.flip) mirror(I, x1, x2, px, ry);
    const double zs = pz * I.scale;
    keep = e.cls >= 0 && e.cls < n_cls;
    if (dataset == 0) {
      // dict objects with rotation_y are level 'DontCare' (truncation -1): the level test never fires
      keep = keep && !(zs < min_depth);
      keep = keep && !(e.cls == 0 ? r[R_LIDAR] <= 100.0 : r[R_LIDAR] <= 50.0);
    } else {
      keep = keep && !(r[R_BEHIND] != 0.0 || zs < min_depth);
      keep = keep && !(r[R_VALID] == 0.0 || r[R_LIDAR] == 0.0 || r[R_DERR] >= 0.5);
      keep = keep && !(r[R_TRUNC] >= 0.75 || (r[R_VIS] <= 0.25 && r[R_VIS] != -1.0));
    }
    // 3D centre = pos - (0, h/2, 0)
    const double cx = px - 0.0, cy = py - h / 2.0, cz = pz - 0.0;
    project_centre(I, cx, cy, cz, e);
    double bcx, bcy, bw, bh;  // the mapped box as xywh, in the precision `bboxes` is divided in
    float X1f = 0.f, X2f = 0.f;
    if (dataset == 0) {
      corner_box(I, h, w, l, ry, cx, cy, cz, e, bcx, bcy, bw, bh);
    } else {
      annotated_box(I, x1, y1, x2, y2, e, X1f, X2f);
      bcx = (double)e.c2x;
      bcy = (double)e.c2y;
      bw = (double)e.s2w;
      bh = (double)e.s2h;
    }
    keep = keep && centre_inside(e, out_w, out_h);
    keep = keep && !(zs > max_depth);
    if (keep) {
      unit_box(e, bcx, bcy, bw, bh, out_w, out_h);
      // the heading's pixel column is the box centre: Waymo's annotated, mirrored box; Omni3D's box array after the crop map, which
      // load_object overwrites in place
      const float ub = dataset == 0 ? ((float)x1 + (float)x2) / 2.f : (X1f + X2f) / 2.f;
      if (I.flip && dataset == 0)
        heading_f32(I, ry, ub, e);
      else
        heading_f64(I, ry, ub, e);
      size_and_depth(I, mean_size, h, w, l, cx, cy, cz, zs, use_camera_dis, e);
    }
  }
  emit_rows(I, b, keep, e, max_objs, out_w, out_h, I.flip != 0, o, counts, calib, ratio_pad);
}

}  // namespace

extern "C" {

int y3d_json3d_encode_labels(const double* rec, const int* img_i, const double* img_f, int B, int dataset, int out_w, int out_h,
                             double min_depth, double max_depth, int use_camera_dis, const double* mean_size, int n_cls, int max_objs,
                             int64_t* cls, double* bboxes, float* center_2d, float* size_2d, double* center_3d, double* size_3d,
                             double* depth, int64_t* heading_bin, double* heading_res, float* batch_idx, int* counts, double* calib,
                             double* ratio_pad, void* stream) {
  Y3D_CHECK(B >= 1 && rec && img_i && img_f && mean_size && n_cls >= 1, "json3d_encode_labels: bad arguments");
  Y3D_CHECK(dataset == 0 || dataset == 1, "json3d_encode_labels: dataset %d (0 Waymo, 1 Omni3D)", dataset);
  LabelOut o{cls, bboxes, center_2d, size_2d, center_3d, size_3d, depth, heading_bin, heading_res, batch_idx};
  if (int rc = check_encode_args("json3d_encode_labels", max_objs, out_w, out_h, o, counts, calib, ratio_pad)) return rc;
  hipLaunchKernelGGL(json3d_labels_kernel, dim3(B), dim3(128), 0, (hipStream_t)stream, rec, img_i, img_f, dataset, out_w, out_h, min_depth,
                     max_depth, use_camera_dis, mean_size, n_cls, max_objs, o, counts, calib, ratio_pad);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

}  // extern "C"
