// The frame the 3D label encoders (kitti_labels.hip, json3d_labels.hip) and the batch plans over a resident split (kitti_cache.hip,
// json3d_cache.hip) share, defined once: the per-image record, the per-lane result and its way into the static rows, the arithmetic
// the three datasets have in common, the plan kernel and the launchers' checks.
//
// Encoders: one workgroup per image, one lane per candidate.  Wave 0 holds the primary frame's candidates (its first min(n, max_objs)),
// wave 1 the mixup partner's (its first min(n2, max_objs - that count), counted before filtering).  Every lane runs its dataset's
// filter chain, then emit_rows writes the survivors to the image's rows [b * max_objs, b * max_objs + count) in record order, primary
// first; the rest of the image's rows get batch_idx = -1 and zeros.
//
// The functions below restate numpy arithmetic operation by operation: every cast and every transcendental call is where the
// reference's dtypes put it.  Contraction is off from here to the end of the including source so each product rounds where numpy's does.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int L3_IMGF = 19;  // per-image doubles: P2 (12), trans (6), scale
constexpr int L3_IMGI = 7;   // per-image ints: primary start, primary candidates, partner start, partner candidates, flip, width, height
constexpr int L3_DRAW = 16;  // draw columns of both plans: pos, partner (-1: none), flip, scale, trans (6), trans_inv (6)

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

// image b's row of img_i / img_f.  The calibration is the (flipped or not) one of the image: KITTI's holds float32 values, the JSON
// datasets' float64 as read and float32 values once mirrored
struct ImageRec {
  int start0, start1, n0, n1, flip;
  double img_w, img_h, p00, p01, p02, p03, p10, p11, p12, p13, t00, t01, t02, t10, t11, t12, scale;
  __device__ __forceinline__ ImageRec(const int* __restrict__ img_i, const double* __restrict__ img_f, int b, int max_objs) {
    const int* ii = img_i + (size_t)b * L3_IMGI;
    const double* fi = img_f + (size_t)b * L3_IMGF;
    start0 = ii[0], start1 = ii[2];
    n0 = max(min(ii[1], max_objs), 0);
    n1 = ii[3] > 0 ? min(ii[3], max_objs - n0) : 0;
    flip = ii[4];
    img_w = (double)ii[5], img_h = (double)ii[6];
    p00 = fi[0], p01 = fi[1], p02 = fi[2], p03 = fi[3], p10 = fi[4], p11 = fi[5], p12 = fi[6], p13 = fi[7];
    t00 = fi[12], t01 = fi[13], t02 = fi[14], t10 = fi[15], t11 = fi[16], t12 = fi[17];
    scale = fi[18];
  }
  __device__ __forceinline__ bool live(int wave, int lane) const { return wave == 0 ? lane < n0 : lane < n1; }
  __device__ __forceinline__ size_t row(int wave, int lane) const { return (size_t)((wave == 0 ? start0 : start1) + lane); }
};

// what a surviving lane writes
struct Encoded {
  int cls = 0, hbin = 0;
  double bb[4] = {0, 0, 0, 0}, c3x = 0, c3y = 0, s3[3] = {0, 0, 0}, dep = 0, hres = 0;
  float c2x = 0, c2y = 0, s2w = 0, s2h = 0;
};

// numpy's float remainder (result takes the divisor's sign)
__device__ __forceinline__ float py_mod(float a, float m) {
  float r = fmodf(a, m);
  if (r != 0.f && ((r < 0.f) != (m < 0.f))) r += m;
  return r;
}
__device__ __forceinline__ double py_mod(double a, double m) {
  double r = fmod(a, m);
  if (r != 0.0 && ((r < 0.0) != (m < 0.0))) r += m;
  return r;
}

// mirror about the original width: the box (stored back as float32), the heading, the position; both frames of a mixup pair have the
// primary's size
__device__ __forceinline__ void mirror(const ImageRec& I, double& x1, double& x2, double& px, double& ry) {
  const double f1 = (double)(float)(I.img_w - x2), f2 = (double)(float)(I.img_w - x1);
  x1 = f1;
  x2 = f2;
  ry = M_PI - ry;
  if (ry > M_PI) ry -= 2.0 * M_PI;
  if (ry < -M_PI) ry += 2.0 * M_PI;
  px = -px;
}

// the 3D centre (cx, cy, cz) projected through P2 and divided by its z, cast to float32, then through the crop map.  The caller forms
// the centre: KITTI adds (0, -h/2, 0) to the position, the JSON datasets subtract (0, h/2, 0), and the two differ in the sign of a zero
__device__ __forceinline__ void project_centre(const ImageRec& I, double cx, double cy, double cz, Encoded& e) {
  const double u = (cx * I.p00 + cy * I.p01 + cz * I.p02 + I.p03) / cz;
  const double v = (cx * I.p10 + cy * I.p11 + cz * I.p12 + I.p13) / cz;
  const double uf = (double)(float)u, vf = (double)(float)v;
  e.c3x = I.t00 * uf + I.t01 * vf + I.t02;
  e.c3y = I.t10 * uf + I.t11 * vf + I.t12;
}

// astype(int32) truncates toward zero: the centre's integer lies in [0, W) iff -1 < x < W (NaN and overflow fail too)
__device__ __forceinline__ bool centre_inside(const Encoded& e, int out_w, int out_h) {
  return (e.c3x > -1.0 && e.c3x < (double)out_w) && (e.c3y > -1.0 && e.c3y < (double)out_h);
}

// the annotated box through the crop map, stored back into its float32 array -> centre_2d / size_2d; X1, X2: the mapped x corners
__device__ __forceinline__ void annotated_box(const ImageRec& I, double x1, double y1, double x2, double y2, Encoded& e, float& X1, float& X2) {
  X1 = (float)(I.t00 * x1 + I.t01 * y1 + I.t02);
  X2 = (float)(I.t00 * x2 + I.t01 * y2 + I.t02);
  const float Y1 = (float)(I.t10 * x1 + I.t11 * y1 + I.t12), Y2 = (float)(I.t10 * x2 + I.t11 * y2 + I.t12);
  e.c2x = (X1 + X2) / 2.f;
  e.c2y = (Y1 + Y2) / 2.f;
  e.s2w = X2 - X1;
  e.s2h = Y2 - Y1;
}

// `bboxes`: the mapped box as xywh, in the precision it is held in, over the resolution, clipped to [0, 1]
__device__ __forceinline__ void unit_box(Encoded& e, double bcx, double bcy, double bw, double bh, int out_w, int out_h) {
  e.bb[0] = fmin(fmax(bcx / (double)out_w, 0.0), 1.0);
  e.bb[1] = fmin(fmax(bcy / (double)out_h, 0.0), 1.0);
  e.bb[2] = fmin(fmax(bw / (double)out_w, 0.0), 1.0);
  e.bb[3] = fmin(fmax(bh / (double)out_h, 0.0), 1.0);
}

// heading: ry2alpha at the pixel column ub, wrapped once in ry2alpha and once more in __getitem__, then 12-bin angle2class.
// heading_f32: a python-float ry against a float32 calibration (KITTI; Waymo mirrored): numpy computes all of it in float32
__device__ __forceinline__ void heading_f32(const ImageRec& I, double ry, float ub, Encoded& e) {
  const float pi_f = (float)M_PI, two_pi_f = (float)(2.0 * M_PI);
  const double apc = 2.0 * M_PI / 12.0;
  float alpha = (float)ry - atan2f(ub - (float)I.p02, (float)I.p00);
  for (int k = 0; k < 2; ++k) {
    if (alpha > pi_f) alpha -= two_pi_f;
    if (alpha < -pi_f) alpha += two_pi_f;
  }
  const float a = py_mod(alpha, two_pi_f);
  const float shifted = py_mod(a + (float)(apc / 2.0), two_pi_f);
  e.hbin = (int)(shifted / (float)apc);
  e.hres = (double)(shifted - (float)(e.hbin * apc + apc / 2.0));
}
// heading_f64: a float64 ry (Omni3D) or a float64 calibration (unmirrored): float64, the arctan2 alone float32 when mirrored
__device__ __forceinline__ void heading_f64(const ImageRec& I, double ry, float ub, Encoded& e) {
  const double apc = 2.0 * M_PI / 12.0;
  const double at = I.flip ? (double)atan2f(ub - (float)I.p02, (float)I.p00) : atan2((double)ub - I.p02, I.p00);
  double alpha = ry - at;
  for (int k = 0; k < 2; ++k) {
    if (alpha > M_PI) alpha -= 2.0 * M_PI;
    if (alpha < -M_PI) alpha += 2.0 * M_PI;
  }
  const double a = py_mod(alpha, 2.0 * M_PI);
  const double shifted = py_mod(a + apc / 2.0, 2.0 * M_PI);
  e.hbin = (int)(shifted / apc);
  e.hres = shifted - (e.hbin * apc + apc / 2.0);
}

// size residual against the class mean (the dimensions are float32 in the reference's array) and the depth: the scaled z, or the
// scaled centre's distance to the camera
__device__ __forceinline__ void size_and_depth(const ImageRec& I, const double* __restrict__ mean_size, double h, double w, double l, double cx,
                                               double cy, double cz, double zs, int use_camera_dis, Encoded& e) {
  const double* ms = mean_size + e.cls * 3;
  e.s3[0] = (double)(float)h - ms[0];
  e.s3[1] = (double)(float)w - ms[1];
  e.s3[2] = (double)(float)l - ms[2];
  const double s = I.scale;
  e.dep = use_camera_dis ? sqrt(cx * s * (cx * s) + cy * s * (cy * s) + cz * s * (cz * s)) : zs;
}

// The tail of both encoders, called by all 128 threads of image b's workgroup: ordered compaction (rank within the wave by ballot +
// popcount, wave 1 behind wave 0's survivors through one LDS word each), the survivors' rows, the padding rows, `counts`, and the
// batch's calibration row (cu, cv, fu, fv, tx, ty) x the resolution ratio with `ratio_pad`.  tx_f32: tx / ty are divided in float32
// (a float32 calibration: KITTI always, the JSON datasets when mirrored)
__device__ __forceinline__ void emit_rows(const ImageRec& I, int b, bool keep, const Encoded& e, int max_objs, int out_w, int out_h, bool tx_f32,
                                          const LabelOut& o, int* __restrict__ counts, double* __restrict__ calib,
                                          double* __restrict__ ratio_pad) {
  __shared__ int kept[2];  // one pair per kernel: a kernel calls this once (a second call would need a barrier before it reuses the words)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const unsigned long long m = __ballot(keep);  // this wave's survivors
  const int rank = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) kept[wave] = __popcll(m);
  __syncthreads();
  const int base0 = kept[0];
  const int count = kept[0] + kept[1];

  const size_t row0 = (size_t)b * max_objs;
  if (keep) {
    const size_t r = row0 + (wave == 0 ? 0 : base0) + rank;
    o.cls[r] = e.cls;
    for (int k = 0; k < 4; ++k) o.bboxes[r * 4 + k] = e.bb[k];
    o.center_2d[r * 2] = e.c2x;
    o.center_2d[r * 2 + 1] = e.c2y;
    o.size_2d[r * 2] = e.s2w;
    o.size_2d[r * 2 + 1] = e.s2h;
    o.center_3d[r * 2] = e.c3x;
    o.center_3d[r * 2 + 1] = e.c3y;
    for (int k = 0; k < 3; ++k) o.size_3d[r * 3 + k] = e.s3[k];
    o.depth[r] = e.dep;
    o.heading_bin[r] = e.hbin;
    o.heading_res[r] = e.hres;
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
    const double r0 = (double)out_w / I.img_w, r1 = (double)out_h / I.img_h;
    const double tx = tx_f32 ? (double)(float)(I.p03 / -I.p00) : I.p03 / -I.p00;
    const double ty = tx_f32 ? (double)(float)(I.p13 / -I.p11) : I.p13 / -I.p11;
    double* c = calib + (size_t)b * 6;
    c[0] = I.p02 * r0;
    c[1] = I.p12 * r1;
    c[2] = I.p00 * r0;
    c[3] = I.p11 * r1;
    c[4] = tx * r0;
    c[5] = ty * r1;
    double* rp = ratio_pad + (size_t)b * 4;
    rp[0] = r0;
    rp[1] = r1;
    rp[2] = 0.0;
    rp[3] = 0.0;
  }
}

// the encoders' launcher checks behind each entry's own test of its inputs (inline: a source that launches no encoder leaves it unused)
inline int check_encode_args(const char* who, int max_objs, int out_w, int out_h, const LabelOut& o, const int* counts, const double* calib,
                             const double* ratio_pad) {
  Y3D_CHECK(max_objs >= 1 && max_objs <= 64, "%s: max_objs %d (1 .. 64 supported)", who, max_objs);
  Y3D_CHECK(out_w >= 1 && out_h >= 1, "%s: bad resolution %d x %d", who, out_w, out_h);
  Y3D_CHECK(o.cls && o.bboxes && o.center_2d && o.size_2d && o.center_3d && o.size_3d && o.depth && o.heading_bin && o.heading_res &&
                o.batch_idx && counts && calib && ratio_pad,
            "%s: null output", who);
  return Y3D_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Batch plan over a resident split: one table of random draws -> the per-image tables y3d_kitti_image_aug (post.hip) and the label
// encoder take, so nothing but the draws crosses PCIe.  One thread per image, copies only (the float32 -> float64 widening of
// KITTI's calibration is exact).  STAGED: the draws carry, behind the shared columns, the byte offset of the primary's frame and of
// the partner's in a per-batch staging buffer (-1: the frame lies in the arena, whose img_off is then read; it holds -1 otherwise)
// ------------------------------------------------------------------------------------------------------------------------------
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

template <typename P2T, bool STAGED>
__global__ void __launch_bounds__(64) plan3d_kernel(const int64_t* __restrict__ img_off, const int* __restrict__ frame_hw,
                                                    const int* __restrict__ rec_span, const P2T* __restrict__ P2, const unsigned char* arena,
                                                    const unsigned char* stage, const double* __restrict__ draws, int B, PlanOut o) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* d = draws + (size_t)b * (STAGED ? L3_DRAW + 2 : L3_DRAW);
  const int pos = (int)d[0], par = (int)d[1];  // both, and the staging offsets, checked against the table on the host
  const int fl = d[2] != 0.0 ? 1 : 0;
  const int H = frame_hw[pos * 2], W = frame_hw[pos * 2 + 1];
  const unsigned char *s0, *s1 = nullptr;
  if (STAGED) {
    s0 = d[16] >= 0.0 ? stage + (int64_t)d[16] : arena + img_off[pos];
    if (par >= 0) s1 = d[17] >= 0.0 ? stage + (int64_t)d[17] : arena + img_off[par];
  } else {
    s0 = arena + img_off[pos];
    if (par >= 0) s1 = arena + img_off[par];
  }
  o.src[b] = s0;
  o.src2[b] = s1;
  o.hw[b * 2] = H;
  o.hw[b * 2 + 1] = W;
  o.flip[b] = fl;
  o.mixed[b] = par >= 0 ? 1 : 0;
  for (int k = 0; k < 6; ++k) o.trans_inv[b * 6 + k] = d[10 + k];
  int* ii = o.img_i + (size_t)b * L3_IMGI;
  const int row0 = rec_span[pos * 2], n0 = rec_span[pos * 2 + 1];
  ii[0] = row0;
  ii[1] = n0;
  ii[2] = par >= 0 ? rec_span[par * 2] : row0 + n0;
  ii[3] = par >= 0 ? rec_span[par * 2 + 1] : 0;
  ii[4] = fl;
  ii[5] = W;
  ii[6] = H;
  double* f = o.img_f + (size_t)b * L3_IMGF;
  const P2T* P = P2 + ((size_t)pos * 2 + fl) * 12;
  for (int k = 0; k < 12; ++k) f[k] = (double)P[k];
  for (int k = 0; k < 6; ++k) f[12 + k] = d[4 + k];
  f[18] = d[3];
}

// refuses, from the host copy of the draws (rows of `width` doubles), a position or partner the kernel could not index the tables with
inline int check_draw_positions(const char* who, const double* draws_host, int B, int width, int N) {
  for (int b = 0; b < B; ++b) {
    const double pos = draws_host[(size_t)b * width], par = draws_host[(size_t)b * width + 1];
    Y3D_CHECK(pos >= 0.0 && pos < (double)N && pos == (double)(int)pos, "%s: image %d: position %g outside [0, %d)", who, b, pos, N);
    Y3D_CHECK(par == -1.0 || (par >= 0.0 && par < (double)N && par == (double)(int)par),
              "%s: image %d: partner %g is neither -1 nor in [0, %d)", who, b, par, N);
  }
  return Y3D_OK;
}

}  // namespace
