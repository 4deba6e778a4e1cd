// Label side of WaymoDataset.__getitem__ (data/datasets/waymo.py:186-290, load_object :292-372) and Omni3Dataset.__getitem__
// (data/datasets/omni3d.py:175-279, load_object :281-352) + their collate_fn on the device, after the plan of kitti_labels.hip: one
// workgroup per image, one lane per candidate object.  Wave 0 holds the primary frame's candidates (its first min(n, max_objs)
// objects), wave 1 the mixup partner's (its first min(n2, max_objs - that count), counted before filtering).  Every lane runs the
// dataset's filter chain, then an ordered compaction (ballot + popcount within a wave, one LDS word between the waves) writes the
// survivors to the image's static rows [b * max_objs, b * max_objs + count) in annotation order, primary first; the rest of the
// image's rows get batch_idx = -1 and zeros.
//
// Precision follows the reference operation by operation.  Positions, dimensions and ry are float64 (they come from JSON); the
// annotated box is float32.  The calibration is float64 as read and float32 once mirrored (Calibration.flip), so tx / ty and the
// heading's arctan2 are float32 exactly when the image is mirrored.  Waymo's box is recomputed from the eight corners that
// keypoint_utils.get_object_keypoints builds in float32 (rotation from float32 sin / cos, corners cast to float32, three-term sums
// accumulated in j order) and adds to the float64 centre; every point is cast to float32 before it goes through the crop matrix.
// Contraction is off so each product rounds where numpy's / torch's does.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int JL_REC = 24;    // packed object record (see y3d.h)
constexpr int JL_IMGF = 19;   // per-image doubles: P2 (12), trans (6), scale
constexpr int JL_IMGI = 7;    // per-image ints: primary start, primary objects, partner start, partner objects, flip, width, height

enum { R_CLS = 0, R_X1, R_Y1, R_X2, R_Y2, R_H, R_W, R_L, R_PX, R_PY, R_PZ, R_RY, R_LIDAR, R_BEHIND, R_VALID, R_DERR, R_TRUNC, R_VIS };

struct LabelOut {
  int64_t* cls;
  double* bboxes;
  float* center_2d;
  float* size_2d;
  double* center_3d;
  double* size_3d;
  double* depth;
  int64_t* heading_bin;
  double* heading_res;
  float* batch_idx;
};

// numpy's float remainder (result takes the divisor's sign)
__device__ __forceinline__ float py_mod_f32(float a, float m) {
  float r = fmodf(a, m);
  if (r != 0.f && ((r < 0.f) != (m < 0.f))) r += m;
  return r;
}
__device__ __forceinline__ double py_mod_f64(double a, double m) {
  double r = fmod(a, m);
  if (r != 0.0 && ((r < 0.0) != (m < 0.0))) r += m;
  return r;
}

__global__ void __launch_bounds__(128) json3d_labels_kernel(const double* __restrict__ rec, const int* __restrict__ img_i,
                                                          const double* __restrict__ img_f, int dataset, int out_w, int out_h,
                                                          double min_depth, double max_depth, int use_camera_dis,
                                                          const double* __restrict__ mean_size, int n_cls, int max_objs, LabelOut o,
                                                          int* __restrict__ counts, double* __restrict__ calib,
                                                          double* __restrict__ ratio_pad) {
  __shared__ int kept[2];
  const int b = blockIdx.x;
  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int* ii = img_i + (size_t)b * JL_IMGI;
  const double* fi = img_f + (size_t)b * JL_IMGF;
  const int n0 = max(min(ii[1], max_objs), 0);
  const int n1 = ii[3] > 0 ? min(ii[3], max_objs - n0) : 0;
  const int flip = ii[4];
  const double img_w = (double)ii[5], img_h = (double)ii[6];
  // the calibration: float64 as read from the JSON, float32 values once mirrored
  const double p00 = fi[0], p01 = fi[1], p02 = fi[2], p03 = fi[3];
  const double p10 = fi[4], p11 = fi[5], p12 = fi[6], p13 = fi[7];
  const double t00 = fi[12], t01 = fi[13], t02 = fi[14], t10 = fi[15], t11 = fi[16], t12 = fi[17];
  const double scale = fi[18];

  const int cand = lane;
  const bool live = wave == 0 ? cand < n0 : cand < n1;
  bool keep = false;
  int cls = 0;
  double bb[4] = {0, 0, 0, 0}, c3x = 0, c3y = 0, dep = 0, s3[3] = {0, 0, 0}, hres = 0;
  float c2x = 0, c2y = 0, s2w = 0, s2h = 0;
  int hbin = 0;
  if (live) {
    const double* r = rec + (size_t)(ii[wave == 0 ? 0 : 2] + cand) * JL_REC;
    cls = (int)r[R_CLS];
    double x1 = r[R_X1], x2 = r[R_X2];
    const double y1 = r[R_Y1], y2 = r[R_Y2];
    const double h = r[R_H], w = r[R_W], l = r[R_L];
    double px = r[R_PX], ry = r[R_RY];
    const double py = r[R_PY], pz = r[R_PZ];
    if (flip) {  // mirror about the original width; both frames of a mixup pair have the primary's size
      const double f1 = (double)(float)(img_w - x2), f2 = (double)(float)(img_w - x1);
      x1 = f1;
      x2 = f2;
      ry = M_PI - ry;
      px = -px;
      if (ry > M_PI) ry -= 2.0 * M_PI;
      if (ry < -M_PI) ry += 2.0 * M_PI;
    }
    const double zs = pz * scale;
    keep = cls >= 0 && cls < n_cls;
    if (dataset == 0) {
      // dict objects with rotation_y are level 'DontCare' (truncation -1): the level test never fires
      keep = keep && !(zs < min_depth);
      keep = keep && !(cls == 0 ? r[R_LIDAR] <= 100.0 : r[R_LIDAR] <= 50.0);
    } else {
      keep = keep && !(r[R_BEHIND] != 0.0 || zs < min_depth);
      keep = keep && !(r[R_VALID] == 0.0 || r[R_LIDAR] == 0.0 || r[R_DERR] >= 0.5);
      keep = keep && !(r[R_TRUNC] >= 0.75 || (r[R_VIS] <= 0.25 && r[R_VIS] != -1.0));
    }
    // 3D centre = pos - (0, h/2, 0), projected through P2 and divided by its z, cast to float32, then through the crop map
    const double cx = px - 0.0, cy = py - h / 2.0, cz = pz - 0.0;
    const double u = (cx * p00 + cy * p01 + cz * p02 + p03) / cz;
    const double v = (cx * p10 + cy * p11 + cz * p12 + p13) / cz;
    const double uf = (double)(float)u, vf = (double)(float)v;
    c3x = t00 * uf + t01 * vf + t02;
    c3y = t10 * uf + t11 * vf + t12;
    double bcx, bcy, bw, bh;  // the mapped box as xywh, in the precision `bboxes` is divided in
    float X1f = 0.f, X2f = 0.f;
    if (dataset == 0) {
      // recompute_bbox_2d: corners of get_object_keypoints(centre, (h, w, l), ry), rotation Rx(pi/2) Ry(-ry) Rz(0) in float32
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
        const double ku = (kx * p00 + ky * p01 + kz * p02 + p03) / kz;
        const double kv = (kx * p10 + ky * p11 + kz * p12 + p13) / kz;
        umin = fmin(umin, ku);
        umax = fmax(umax, ku);
        vmin = fmin(vmin, kv);
        vmax = fmax(vmax, kv);
      }
      const double a0 = (double)(float)umin, a1 = (double)(float)vmin, a2 = (double)(float)umax, a3 = (double)(float)vmax;
      const double X1 = t00 * a0 + t01 * a1 + t02, Y1 = t10 * a0 + t11 * a1 + t12;
      const double X2 = t00 * a2 + t01 * a3 + t02, Y2 = t10 * a2 + t11 * a3 + t12;
      bcx = (X1 + X2) / 2.0;
      bcy = (Y1 + Y2) / 2.0;
      bw = X2 - X1;
      bh = Y2 - Y1;
      c2x = (float)bcx;
      c2y = (float)bcy;
      s2w = (float)bw;
      s2h = (float)bh;
    } else {
      // the annotated box through the crop map, stored back into its float32 array
      X1f = (float)(t00 * x1 + t01 * y1 + t02);
      X2f = (float)(t00 * x2 + t01 * y2 + t02);
      const float Y1f = (float)(t10 * x1 + t11 * y1 + t12), Y2f = (float)(t10 * x2 + t11 * y2 + t12);
      c2x = (X1f + X2f) / 2.f;
      c2y = (Y1f + Y2f) / 2.f;
      s2w = X2f - X1f;
      s2h = Y2f - Y1f;
      bcx = (double)c2x;
      bcy = (double)c2y;
      bw = (double)s2w;
      bh = (double)s2h;
    }
    // astype(int32) truncates toward zero: the integer lies in [0, W) iff -1 < x < W (NaN and overflow fail too)
    keep = keep && (c3x > -1.0 && c3x < (double)out_w) && (c3y > -1.0 && c3y < (double)out_h);
    keep = keep && !(zs > max_depth);
    if (keep) {
      bb[0] = fmin(fmax(bcx / (double)out_w, 0.0), 1.0);
      bb[1] = fmin(fmax(bcy / (double)out_h, 0.0), 1.0);
      bb[2] = fmin(fmax(bw / (double)out_w, 0.0), 1.0);
      bb[3] = fmin(fmax(bh / (double)out_h, 0.0), 1.0);
      // heading: ry2alpha at the box centre (Waymo: the annotated, mirrored box; Omni3D: its box array after the crop map, which
      // load_object overwrites in place), wrapped twice, 12-bin angle2class.  float32 where numpy's operands are
      const float ub = dataset == 0 ? ((float)x1 + (float)x2) / 2.f : (X1f + X2f) / 2.f;
      const double apc = 2.0 * M_PI / 12.0;
      if (flip && dataset == 0) {  // python-float ry against the mirrored float32 calibration: all float32
        const float pi_f = (float)M_PI, two_pi_f = (float)(2.0 * M_PI);
        float alpha = (float)ry - atan2f(ub - (float)p02, (float)p00);
        for (int k = 0; k < 2; ++k) {
          if (alpha > pi_f) alpha -= two_pi_f;
          if (alpha < -pi_f) alpha += two_pi_f;
        }
        const float a = py_mod_f32(alpha, two_pi_f);
        const float shifted = py_mod_f32(a + (float)(apc / 2.0), two_pi_f);
        hbin = (int)(shifted / (float)apc);
        hres = (double)(shifted - (float)(hbin * apc + apc / 2.0));
      } else {  // float64 ry (Omni3D) or float64 calibration (unmirrored): float64, the arctan2 alone float32 when mirrored
        const double at = flip ? (double)atan2f(ub - (float)p02, (float)p00) : atan2((double)ub - p02, p00);
        double alpha = ry - at;
        for (int k = 0; k < 2; ++k) {
          if (alpha > M_PI) alpha -= 2.0 * M_PI;
          if (alpha < -M_PI) alpha += 2.0 * M_PI;
        }
        const double a = py_mod_f64(alpha, 2.0 * M_PI);
        const double shifted = py_mod_f64(a + apc / 2.0, 2.0 * M_PI);
        hbin = (int)(shifted / apc);
        hres = shifted - (hbin * apc + apc / 2.0);
      }
      const double* ms = mean_size + cls * 3;
      s3[0] = (double)(float)h - ms[0];
      s3[1] = (double)(float)w - ms[1];
      s3[2] = (double)(float)l - ms[2];
      dep = use_camera_dis ? sqrt(cx * scale * (cx * scale) + cy * scale * (cy * scale) + cz * scale * (cz * scale)) : zs;
    }
  }

  // ordered compaction: rank within the wave, wave 1 behind wave 0's survivors
  const unsigned long long m = __ballot(keep);  // this wave's survivors
  const int rank = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) kept[wave] = __popcll(m);
  __syncthreads();
  const int base0 = kept[0];
  const int count = kept[0] + kept[1];

  const size_t row0 = (size_t)b * max_objs;
  if (keep) {
    const size_t r = row0 + (wave == 0 ? 0 : base0) + rank;
    o.cls[r] = cls;
    for (int k = 0; k < 4; ++k) o.bboxes[r * 4 + k] = bb[k];
    o.center_2d[r * 2] = c2x;
    o.center_2d[r * 2 + 1] = c2y;
    o.size_2d[r * 2] = s2w;
    o.size_2d[r * 2 + 1] = s2h;
    o.center_3d[r * 2] = c3x;
    o.center_3d[r * 2 + 1] = c3y;
    for (int k = 0; k < 3; ++k) o.size_3d[r * 3 + k] = s3[k];
    o.depth[r] = dep;
    o.heading_bin[r] = hbin;
    o.heading_res[r] = hres;
    o.batch_idx[r] = (float)b;
  }
  for (int j = count + t; j < max_objs; j += 128) {  // padding rows
    const size_t r = row0 + j;
    o.cls[r] = 0;
    for (int k = 0; k < 4; ++k) o.bboxes[r * 4 + k] = 0.0;
    o.center_2d[r * 2] = o.center_2d[r * 2 + 1] = 0.f;
    o.size_2d[r * 2] = o.size_2d[r * 2 + 1] = 0.f;
    o.center_3d[r * 2] = o.center_3d[r * 2 + 1] = 0.0;
    for (int k = 0; k < 3; ++k) o.size_3d[r * 3 + k] = 0.0;
    o.depth[r] = 0.0;
    o.heading_bin[r] = 0;
    o.heading_res[r] = 0.0;
    o.batch_idx[r] = -1.f;
  }
  if (t == 0) {
    counts[b] = count;
    // calibration rows of the batch: (cu, cv, fu, fv, tx, ty) x the resolution ratio; tx / ty divided in the calibration's dtype
    const double r0 = (double)out_w / img_w, r1 = (double)out_h / img_h;
    const double tx = flip ? (double)(float)(p03 / -p00) : p03 / -p00;
    const double ty = flip ? (double)(float)(p13 / -p11) : p13 / -p11;
    double* c = calib + (size_t)b * 6;
    c[0] = p02 * r0;
    c[1] = p12 * r1;
    c[2] = p00 * r0;
    c[3] = p11 * r1;
    c[4] = tx * r0;
    c[5] = ty * r1;
    double* rp = ratio_pad + (size_t)b * 4;
    rp[0] = r0;
    rp[1] = r1;
    rp[2] = 0.0;
    rp[3] = 0.0;
  }
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
  Y3D_CHECK(max_objs >= 1 && max_objs <= 64, "json3d_encode_labels: max_objs %d (1 .. 64 supported)", max_objs);
  Y3D_CHECK(out_w >= 1 && out_h >= 1, "json3d_encode_labels: bad resolution %d x %d", out_w, out_h);
  Y3D_CHECK(cls && bboxes && center_2d && size_2d && center_3d && size_3d && depth && heading_bin && heading_res && batch_idx && counts &&
                calib && ratio_pad,
            "json3d_encode_labels: null output");
  LabelOut o{cls, bboxes, center_2d, size_2d, center_3d, size_3d, depth, heading_bin, heading_res, batch_idx};
  hipLaunchKernelGGL(json3d_labels_kernel, dim3(B), dim3(128), 0, (hipStream_t)stream, rec, img_i, img_f, dataset, out_w, out_h, min_depth,
                     max_depth, use_camera_dis, mean_size, n_cls, max_objs, o, counts, calib, ratio_pad);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

}  // extern "C"
