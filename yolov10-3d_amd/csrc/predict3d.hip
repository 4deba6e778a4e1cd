// The 3D predictor's row pass: post-processed rows in, what a caller of a mono-3D detector uses out (predict.Predictor3d).
//
// y3d_predict3d_rows — one workgroup of 256 threads per image, the image's K rows walked in chunks of 256.  Per row:
//
//   decode   kitti_row.h's kitti_decode_row, the arithmetic of y3d_kitti_decode (data/datasets/kitti.py:519-576) in its order and
//            precisions, so the 14 values [cls, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, score] are that kernel's bit for bit
//   filter   kept when !(score < conf) (the decode's own rule: a NaN score is kept as there) and, with a class list, when
//            (int)preds[.., 36] is in it (models/yolov10_3D/predict.py:23-25)
//   compact  survivors keep their input (score) order: ballot + popcount within a wave, an LDS prefix over the four waves, a running
//            base across chunks (the scheme of predict_rows_kernel, letterbox.hip)
//   corners  kitti_row.h's kitti_box_corners: Object3d.generate_corners3d (kitti_utils.py:98-114) in float64 from the row's own h, w, l,
//            (x, y, z), ry, y the bottom face, and
//   project  Calibration.corners3d_to_img_boxes' boxes_corner (kitti_utils.py:266-284) with the full 3 x 4 P2:
//              (P2[0] . (X, Y, Z, 1) / P2[2] . (X, Y, Z, 1),  P2[1] . (X, Y, Z, 1) / P2[2] . (X, Y, Z, 1)), divided whatever the sign
//
// The eight corners are unrolled (no run-time indexed private array, so no scratch); a kept row leaves as 27 16-byte stores (its row
// strides of 112, 192 and 128 bytes are multiples of 16).  Slots behind the survivors are zeros in all three outputs.
#include "common.h"
#include "kitti_row.h"

#pragma clang fp contract(off)

namespace {

__global__ void __launch_bounds__(256) predict3d_rows_kernel(const float* __restrict__ preds, int K, const double* __restrict__ calib,
                                                           const double* __restrict__ P2, const double* __restrict__ ratio,
                                                           const double* __restrict__ inv_trans, const double* __restrict__ mean_size,
                                                           int nc, int use_camera_dis, double conf, const int* __restrict__ classes,
                                                           int n_cls, double* __restrict__ rows, double* __restrict__ corners3d,
                                                           double* __restrict__ corners_img, int* __restrict__ counts) {
  __shared__ int wsum[4];
  const int b = blockIdx.x;
  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const double* P = P2 + (size_t)b * 12;
  const double rw = ratio[b * 2], rh = ratio[b * 2 + 1];
  const double* cal = calib + (size_t)b * 6;
  const double* ti = inv_trans ? inv_trans + (size_t)b * 6 : nullptr;
  const float* in = preds + (size_t)b * K * 37;
  double2* orow = (double2*)(rows + (size_t)b * K * 14);
  double2* oc3 = (double2*)(corners3d + (size_t)b * K * 24);
  double2* oci = (double2*)(corners_img + (size_t)b * K * 16);
  int base = 0;
  for (int c0 = 0; c0 < K; c0 += 256) {
    const int k = c0 + t;
    bool keep = false;
    double v[14];
#pragma unroll
    for (int i = 0; i < 14; ++i) v[i] = 0.0;
    if (k < K) {
      const float* r = in + (size_t)k * 37;
      kitti_decode_row(r, cal, rw, rh, ti, mean_size, nc, use_camera_dis, v);
      keep = !(v[13] < conf);
      if (n_cls > 0) {
        const int cid = (int)r[36];
        bool hit = false;
        for (int i = 0; i < n_cls; ++i) hit = hit || (cid == classes[i]);
        keep = keep && hit;
      }
    }
    const unsigned long long m = __ballot(keep);
    const int rank = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < 4; ++w) {
      before += w < wave ? wsum[w] : 0;
      all += wsum[w];
    }
    if (keep) {  // base + before + rank <= k < K
      const size_t j = (size_t)(base + before + rank);
#pragma unroll
      for (int i = 0; i < 7; ++i) orow[j * 7 + i] = make_double2(v[2 * i], v[2 * i + 1]);
      double c3[24], ci[16];
      kitti_box_corners(v[6], v[7], v[8], v[9], v[10], v[11], v[12], P, c3, ci);
#pragma unroll
      for (int i = 0; i < 12; ++i) oc3[j * 12 + i] = make_double2(c3[2 * i], c3[2 * i + 1]);
#pragma unroll
      for (int i = 0; i < 8; ++i) oci[j * 8 + i] = make_double2(ci[2 * i], ci[2 * i + 1]);
    }
    base += all;
    __syncthreads();
  }
  // the slots behind the survivors (the outputs alias no input, so nothing that is still to be read is overwritten)
  const double2 z = make_double2(0.0, 0.0);
  for (int j = base + t; j < K; j += 256) {
#pragma unroll
    for (int i = 0; i < 7; ++i) orow[(size_t)j * 7 + i] = z;
#pragma unroll
    for (int i = 0; i < 12; ++i) oc3[(size_t)j * 12 + i] = z;
#pragma unroll
    for (int i = 0; i < 8; ++i) oci[(size_t)j * 8 + i] = z;
  }
  if (t == 0) counts[b] = base;
}

struct Span {
  const void* p;
  size_t bytes;
};

inline bool overlaps(const Span& a, const Span& b) {
  const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
  return a.bytes && b.bytes && a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

}  // namespace

extern "C" {

int y3d_predict3d_rows(const float* preds, int B, int K, const double* calib, const double* P2, const double* ratio,
                       const double* inv_trans, const double* mean_size, int nc, int use_camera_dis, double conf, const int* classes,
                       int n_cls, double* rows, double* corners3d, double* corners_img, int* counts, void* stream) {
  Y3D_CHECK(preds && calib && P2 && ratio && mean_size && rows && corners3d && corners_img && counts, "predict3d_rows: null argument");
  Y3D_CHECK(B >= 1 && K >= 1 && nc >= 1 && n_cls >= 0 && (n_cls == 0 || classes), "predict3d_rows: bad sizes");
  Y3D_CHECK((((uintptr_t)rows | (uintptr_t)corners3d | (uintptr_t)corners_img) & 15) == 0, "predict3d_rows: outputs must be 16-byte aligned");
  // byte ranges, so that an output overlapping an input at an offset (views into one allocation) is caught too
  const size_t rk = (size_t)B * K;
  const Span ins[] = {{preds, rk * 37 * 4}, {calib, (size_t)B * 48}, {P2, (size_t)B * 96}, {ratio, (size_t)B * 16},
                      {inv_trans, inv_trans ? (size_t)B * 48 : 0}, {mean_size, (size_t)nc * 24}, {classes, (size_t)n_cls * 4}};
  const Span outs[] = {{rows, rk * 14 * 8}, {corners3d, rk * 24 * 8}, {corners_img, rk * 16 * 8}, {counts, (size_t)B * 4}};
  for (int o = 0; o < 4; ++o) {
    for (const Span& i : ins) Y3D_CHECK(!overlaps(outs[o], i), "predict3d_rows: an output overlaps an input");
    for (int q = o + 1; q < 4; ++q) Y3D_CHECK(!overlaps(outs[o], outs[q]), "predict3d_rows: the outputs overlap each other");
  }
  hipLaunchKernelGGL(predict3d_rows_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, preds, K, calib, P2, ratio, inv_trans, mean_size, nc,
                     use_camera_dis, conf, classes, n_cls, rows, corners3d, corners_img, counts);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

}  // extern "C"
