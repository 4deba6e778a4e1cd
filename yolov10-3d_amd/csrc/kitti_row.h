// One row of the KITTI decode (data/datasets/kitti.py:519-576), shared by kitti_decode_kernel (post.hip) and predict3d_rows_kernel
// (predict3d.hip) so that both compute the same bits; its back-projection, alpha2ry and the box corners are functions of their own, which
// the label decode (decode_labels.hip) shares.  The reference promotes the float32 predictions to float64 through the
// calibration constants; the float32 steps (heading angle, sigmoid, exp) are kept in float32 here as there; the size is a float64 sum stored as float32.  The
// library is built with contraction off: the order of the operations below is the result.
#pragma once
#include "common.h"

// Calibration.img_to_rect (kitti_utils.py:241-251) or, with use_camera_dis, camera_dis_to_rect (:286-299): the pixel (u, v) of the
// original image at `depth` (the rect z, or the distance to the camera) -> the point (lx, ly, lz) in the rectified camera frame
__device__ __forceinline__ void kitti_pixel_to_rect(double u, double v, double depth, const double* __restrict__ calib, int use_camera_dis,
                                                    double& lx, double& ly, double& lz) {
  const double cu = calib[0], cv = calib[1], fu = calib[2], fv = calib[3], tx = calib[4], ty = calib[5];
  if (use_camera_dis) {
    const double fd = sqrt((u - cu) * (u - cu) + (v - cv) * (v - cv) + fu * fu);
    lx = ((u - cu) * depth) / fd + tx;
    ly = ((v - cv) * depth) / fd + ty;
    lz = sqrt(depth * depth - lx * lx - ly * ly);
  } else {
    lx = ((u - cu) * depth) / fu + tx;
    ly = ((v - cv) * depth) / fv + ty;
    lz = depth;
  }
}

// Calibration.alpha2ry (kitti_utils.py:311-325) at the pixel column xc
__device__ __forceinline__ double kitti_alpha2ry(double alpha, double xc, double cu, double fu) {
  const double PI_D = 3.14159265358979323846;
  double ry = alpha + atan2(xc - cu, fu);
  if (ry > PI_D) ry -= 2 * PI_D;
  if (ry < -PI_D) ry += 2 * PI_D;
  return ry;
}

// Object3d.generate_corners3d (kitti_utils.py:98-114) from a decoded row's h, w, l, (x, y, z), ry, y the bottom face:
//   xc = (l/2, l/2, -l/2, -l/2) twice, yc = (0, 0, 0, 0, -h, -h, -h, -h), zc = (w/2, -w/2, -w/2, w/2) twice
//   X = cos(ry) xc + sin(ry) zc + x,  Y = yc + y,  Z = -sin(ry) xc + cos(ry) zc + z
// and, when P (the 3 x 4 projection, 12 doubles) is given, Calibration.corners3d_to_img_boxes' boxes_corner (:266-284), divided whatever
// the sign.  The eight corners are unrolled: no run-time indexed private array, so no scratch.  P == nullptr leaves ci untouched.
__device__ __forceinline__ void kitti_box_corners(double h, double w, double l, double x, double y, double z, double ry,
                                                  const double* __restrict__ P, double (&c3)[24], double (&ci)[16]) {
  const double hl = l / 2, hw = w / 2;
  const double cs = cos(ry), sn = sin(ry);
  double p00 = 0, p01 = 0, p02 = 0, p03 = 0, p10 = 0, p11 = 0, p12 = 0, p13 = 0, p20 = 0, p21 = 0, p22 = 0, p23 = 0;
  if (P) {
    p00 = P[0]; p01 = P[1]; p02 = P[2]; p03 = P[3]; p10 = P[4]; p11 = P[5]; p12 = P[6]; p13 = P[7]; p20 = P[8]; p21 = P[9]; p22 = P[10];
    p23 = P[11];
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const double xc = (c & 2) ? -hl : hl;
    const double zc = ((c & 3) == 0 || (c & 3) == 3) ? hw : -hw;
    const double yc = c < 4 ? 0.0 : -h;
    const double X = (cs * xc + sn * zc) + x;
    const double Y = yc + y;
    const double Z = (-sn * xc + cs * zc) + z;
    c3[c * 3 + 0] = X;
    c3[c * 3 + 1] = Y;
    c3[c * 3 + 2] = Z;
    if (P) {
      const double d = ((X * p20 + Y * p21) + Z * p22) + p23;
      ci[c * 2 + 0] = (((X * p00 + Y * p01) + Z * p02) + p03) / d;
      ci[c * 2 + 1] = (((X * p10 + Y * p11) + Z * p12) + p13) / d;
    }
  }
}

// r: the row's 37 float32 values; calib: the image's (cu, cv, fu, fv, tx, ty); rw, rh: its ratio; t: its (2, 3) inverse affine or
// nullptr (the fixed 1242/1280, 375/384 rescale); o: [cls, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, score]
__device__ __forceinline__ void kitti_decode_row(const float* __restrict__ r, const double* __restrict__ calib, double rw, double rh,
                                                 const double* __restrict__ t, const double* __restrict__ mean_size, int nc,
                                                 int use_camera_dis, double (&o)[14]) {
  const double cu = calib[0], fu = calib[2];
  int cid = (int)r[36];
  const int cm = cid < 0 ? 0 : (cid >= nc ? nc - 1 : cid);  // the reference would raise on a label outside the mean-size table
  // heading: first maximum of the 12 bin logits, residual of that bin (decode_helper.py:12-18, float32)
  int bin = 0;
  float best = r[9];
  for (int k = 1; k < 12; ++k) if (r[9 + k] > best) { best = r[9 + k]; bin = k; }
  const float PI_F = 3.14159265358979323846f;
  float ang = (float)bin * (float)(2.0 * 3.14159265358979323846 / 12.0) + r[21 + bin];
  if (ang > PI_F) ang = ang - (float)(2.0 * 3.14159265358979323846);
  const double alpha = (double)ang;
  const double x1 = (double)r[0] / rw, y1 = (double)r[1] / rh, x2 = (double)r[2] / rw, y2 = (double)r[3] / rh;
  const double xc = (x1 + x2) / 2;
  // `dimensions += cls_mean_size[cls]` on a float32 array with a float64 table: numpy adds in float64 and rounds the SUM to float32
  // (adding the table rounded to float32 is one ulp off in about a tenth of the rows)
  const float h = (float)((double)r[6] + mean_size[cm * 3 + 0]), w = (float)((double)r[7] + mean_size[cm * 3 + 1]),
              l = (float)((double)r[8] + mean_size[cm * 3 + 2]);
  const double depth = (double)r[33];
  const double sigma = (double)expf(-r[34]);
  double u, v;
  if (t) {
    u = t[0] * (double)r[4] + t[1] * (double)r[5] + t[2];
    v = t[3] * (double)r[4] + t[4] * (double)r[5] + t[5];
  } else {
    u = (double)((r[4] * 1242.f) / 1280.f);
    v = (double)((r[5] * 375.f) / 384.f);
  }
  double lx, ly, lz;
  kitti_pixel_to_rect(u, v, depth, calib, use_camera_dis, lx, ly, lz);
  ly += (double)h / 2;
  const double ry = kitti_alpha2ry(alpha, xc, cu, fu);
  const float sg = 1.f / (1.f + expf(-r[35]));
  const double score = (double)sg * sigma;
  o[0] = (double)cid; o[1] = alpha; o[2] = x1; o[3] = y1; o[4] = x2; o[5] = y2; o[6] = (double)h; o[7] = (double)w; o[8] = (double)l;
  o[9] = lx; o[10] = ly; o[11] = lz; o[12] = ry; o[13] = score;
}
