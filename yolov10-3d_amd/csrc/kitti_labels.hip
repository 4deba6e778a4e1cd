// Label side of KITTIDataset.__getitem__ (data/datasets/kitti.py:208-405) + collate_fn (:579-599) on the device: one workgroup per
// image, one lane per candidate label line.  Wave 0 holds the primary frame's candidates (its first min(n, max_objs) lines), wave 1
// the mixup partner's (its first min(n2, max_objs - that count) lines).  Every lane runs the reference's filter chain, then an ordered
// compaction (ballot + popcount within a wave, one LDS word between the waves) writes the survivors to the image's static rows
// [b * max_objs, b * max_objs + count) in label-file order, primary first; the rest of the image's rows get batch_idx = -1 and zeros.
//
// Precision follows the reference's numpy arithmetic: boxes and positions are float32 values held in double; mapped box corners,
// centre_2d / size_2d and the whole heading encoding (f32 calibration, python scalars weakly typed) are float32; the projected 3D centre,
// the depth and the size residual are float64.  Contraction is off so each product rounds where numpy's does.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int KL_REC = 16;    // packed label record (see y3d.h)
constexpr int KL_IMGF = 19;   // per-image doubles: P2 (12), trans (6), scale
constexpr int KL_IMGI = 7;    // per-image ints: primary start, primary lines, partner start, partner lines, flip, width, height

enum { R_CLS = 0, R_TRUNC, R_OCC, R_X1, R_Y1, R_X2, R_Y2, R_H, R_W, R_L, R_PX, R_PY, R_PZ, R_RY };

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

// numpy's float remainder (result takes the divisor's sign), in float32
__device__ __forceinline__ float py_mod_f32(float a, float m) {
  float r = fmodf(a, m);
  if (r != 0.f && ((r < 0.f) != (m < 0.f))) r += m;
  return r;
}

__global__ void __launch_bounds__(128) kitti_labels_kernel(const double* __restrict__ rec, const int* __restrict__ img_i,
                                                         const double* __restrict__ img_f, int out_w, int out_h, double min_depth,
                                                         double max_depth, int use_camera_dis, const double* __restrict__ mean_size,
                                                         int n_cls, int max_objs, LabelOut o, int* __restrict__ counts,
                                                         double* __restrict__ calib, double* __restrict__ ratio_pad) {
  __shared__ int kept[2];
  const int b = blockIdx.x;
  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int* ii = img_i + (size_t)b * KL_IMGI;
  const double* fi = img_f + (size_t)b * KL_IMGF;
  const int n0 = min(ii[1], max_objs);
  const int n1 = ii[3] > 0 ? min(ii[3], max_objs - n0) : 0;
  const int flip = ii[4];
  const double img_w = (double)ii[5], img_h = (double)ii[6];
  // the calibration (flipped or not) as the float32 values the reference holds
  const double p00 = fi[0], p01 = fi[1], p02 = fi[2], p03 = fi[3];
  const double p10 = fi[4], p11 = fi[5], p12 = fi[6], p13 = fi[7];
  const double t00 = fi[12], t01 = fi[13], t02 = fi[14], t10 = fi[15], t11 = fi[16], t12 = fi[17];
  const double scale = fi[18];
  const float cu = (float)p02, fu = (float)p00;

  const int cand = lane;
  const bool live = wave == 0 ? cand < n0 : cand < n1;
  bool keep = false;
  int cls = 0;
  double bb[4] = {0, 0, 0, 0}, c3x = 0, c3y = 0, dep = 0, s3[3] = {0, 0, 0};
  float c2x = 0, c2y = 0, s2w = 0, s2h = 0, hres = 0;
  int hbin = 0;
  if (live) {
    const double* r = rec + (size_t)(ii[wave == 0 ? 0 : 2] + cand) * KL_REC;
    cls = (int)r[R_CLS];
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
    if (flip) {  // mirror about the original width; both frames of a mixup pair have the primary's size
      const double f1 = (double)(float)(img_w - x2), f2 = (double)(float)(img_w - x1);
      x1 = f1;
      x2 = f2;
      ry = M_PI - ry;
      if (ry > M_PI) ry -= 2.0 * M_PI;
      if (ry < -M_PI) ry += 2.0 * M_PI;
      px = -px;
    }
    keep = cls >= 0 && cls < n_cls;
    keep = keep && !(unknown || pz * scale < min_depth);
    keep = keep && !(trunc > 0.5 || occ > 2.0);
    // box corners through the crop map, stored back as float32
    const float X1 = (float)(t00 * x1 + t01 * y1 + t02), Y1 = (float)(t10 * x1 + t11 * y1 + t12);
    const float X2 = (float)(t00 * x2 + t01 * y2 + t02), Y2 = (float)(t10 * x2 + t11 * y2 + t12);
    c2x = (X1 + X2) / 2.f;
    c2y = (Y1 + Y2) / 2.f;
    s2w = X2 - X1;
    s2h = Y2 - Y1;
    // 3D centre = pos + (0, -h/2, 0), projected through P2 and divided by the rect z, then through the crop map
    const double cx = px + 0.0, cy = py + (-h / 2.0), cz = pz + 0.0;
    const double u = (cx * p00 + cy * p01 + cz * p02 + p03) / cz;
    const double v = (cx * p10 + cy * p11 + cz * p12 + p13) / cz;
    const double uf = (double)(float)u, vf = (double)(float)v;
    c3x = t00 * uf + t01 * vf + t02;
    c3y = t10 * uf + t11 * vf + t12;
    // astype(int32) truncates toward zero: the integer lies in [0, W) iff -1 < x < W (NaN and overflow fail too)
    keep = keep && (c3x > -1.0 && c3x < (double)out_w) && (c3y > -1.0 && c3y < (double)out_h);
    const double zs = pz * scale;
    keep = keep && !(zs > max_depth);
    if (keep) {
      bb[0] = fmin(fmax((double)c2x / (double)out_w, 0.0), 1.0);
      bb[1] = fmin(fmax((double)c2y / (double)out_h, 0.0), 1.0);
      bb[2] = fmin(fmax((double)s2w / (double)out_w, 0.0), 1.0);
      bb[3] = fmin(fmax((double)s2h / (double)out_h, 0.0), 1.0);
      // heading: ry2alpha at the flipped, untransformed box centre, wrapped, 12-bin angle2class — all float32
      const float ub = ((float)x1 + (float)x2) / 2.f;
      const float pi_f = (float)M_PI, two_pi_f = (float)(2.0 * M_PI);
      float alpha = (float)ry - atan2f(ub - cu, fu);
      for (int k = 0; k < 2; ++k) {  // once in ry2alpha, once more in __getitem__
        if (alpha > pi_f) alpha -= two_pi_f;
        if (alpha < -pi_f) alpha += two_pi_f;
      }
      const double apc = 2.0 * M_PI / 12.0;
      const float a = py_mod_f32(alpha, two_pi_f);
      const float shifted = py_mod_f32(a + (float)(apc / 2.0), two_pi_f);
      hbin = (int)(shifted / (float)apc);
      hres = shifted - (float)(hbin * apc + apc / 2.0);
      const double* ms = mean_size + cls * 3;
      s3[0] = (double)(float)h - ms[0];
      s3[1] = (double)(float)r[R_W] - ms[1];
      s3[2] = (double)(float)r[R_L] - ms[2];
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
    o.heading_res[r] = (double)hres;
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
    // calibration rows of the batch: (cu, cv, fu, fv, tx, ty) of the (flipped) float32 P2 x the resolution ratio
    const double r0 = (double)out_w / img_w, r1 = (double)out_h / img_h;
    const double tx = (double)(float)(p03 / -p00), ty = (double)(float)(p13 / -p11);
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

int y3d_kitti_encode_labels(const double* rec, const int* img_i, const double* img_f, int B, int out_w, int out_h, double min_depth,
                            double max_depth, int use_camera_dis, const double* mean_size, int n_cls, int max_objs, int64_t* cls,
                            double* bboxes, float* center_2d, float* size_2d, double* center_3d, double* size_3d, double* depth,
                            int64_t* heading_bin, double* heading_res, float* batch_idx, int* counts, double* calib, double* ratio_pad,
                            void* stream) {
  Y3D_CHECK(B >= 1 && img_i && img_f && mean_size && n_cls >= 1, "kitti_encode_labels: bad arguments");
  Y3D_CHECK(max_objs >= 1 && max_objs <= 64, "kitti_encode_labels: max_objs %d (1 .. 64 supported)", max_objs);
  Y3D_CHECK(out_w >= 1 && out_h >= 1, "kitti_encode_labels: bad resolution %d x %d", out_w, out_h);
  Y3D_CHECK(cls && bboxes && center_2d && size_2d && center_3d && size_3d && depth && heading_bin && heading_res && batch_idx && counts &&
                calib && ratio_pad,
            "kitti_encode_labels: null output");
  LabelOut o{cls, bboxes, center_2d, size_2d, center_3d, size_3d, depth, heading_bin, heading_res, batch_idx};
  hipLaunchKernelGGL(kitti_labels_kernel, dim3(B), dim3(128), 0, (hipStream_t)stream, rec, img_i, img_f, out_w, out_h, min_depth, max_depth,
                     use_camera_dis, mean_size, n_cls, max_objs, o, counts, calib, ratio_pad);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

}  // extern "C"
