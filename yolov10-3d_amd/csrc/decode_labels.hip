// The labels of a batch back to 3D boxes: `KITTIDataset.decode_batch` (data/datasets/kitti.py:469-513; waymo.py and omni3d.py carry
// identical copies) on the device, with the box corners and their projection that the pictures need.
//
// y3d_decode_labels — one workgroup of ONE wave per image, one lane per label row.  The per-image constants (calibration, ratio,
// inverse affine, projection, original size) sit at addresses that depend on blockIdx alone, so they are scalar loads; the per-row
// label values are the vector side.  Both layouts of the batch builders go through one loop over chunks of 64 candidate rows:
//
//   static   image b's candidates are rows [b * max_objs, b * max_objs + min(counts_in[b], max_objs)), every one of them its own
//            (max_objs = 50: one chunk)
//   ragged   the candidates are all N rows; image b owns those with batch_idx == b, in batch order
//
// and an ordered compaction (ballot + popcount within the wave, a running base across chunks: one wave, so no LDS at all) puts the
// j-th owned row into slot j.  Rows beyond R slots are dropped, counts[b] = min(owned, R); the slots behind are zeros.
//
// Per row, decode_batch line by line, in float64 as numpy computes it there:
//   x = bbox[0] * W; xywh2xyxy (x -+ w / 2, y -+ h / 2) * (W, H, W, H)                                            (:478-480)
//   dimensions = size_3d + cls_mean_size[cls]                                                                      (:482-483)
//   undo_augment: the centre through trans_inv, after affine_transform's rounding of the point to float32 (kitti_utils.py:467-470);
//   otherwise the centre / ratio_pad[i][0]                                                                         (:487-501)
//   img_to_rect or camera_dis_to_rect, y += h / 2, class2angle(to_label_format=True), alpha2ry at x, score = 1     (:491-508)
// The back-projection, alpha2ry and the corners are kitti_row.h's, shared with the prediction decode.  A class outside the mean-size
// table is signalled as y3d_kitti_decode signals it: the row keeps the class it came with in column 0 and takes the nearest table
// entry's size, so nothing is read out of bounds and the caller sees the label (the reference raises an IndexError there).
#include "common.h"
#include "kitti_row.h"

#pragma clang fp contract(off)

namespace {

struct LabelIn {
  const int64_t* cls;
  const double* bboxes;
  const double* center_3d;
  const double* size_3d;
  const double* depth;
  const int64_t* heading_bin;
  const double* heading_res;
  const float* batch_idx;
};

__global__ void __launch_bounds__(64) decode_labels_kernel(LabelIn in, const int* __restrict__ counts_in, int N, int max_objs,
                                                         const double* __restrict__ ori_shape, const double* __restrict__ calib,
                                                         const double* __restrict__ ratio, int ratio_pitch,
                                                         const double* __restrict__ trans_inv, const double* __restrict__ P2,
                                                         const double* __restrict__ mean_size, int nc, int use_camera_dis,
                                                         int undo_augment, int R, double* __restrict__ rows,
                                                         double* __restrict__ corners3d, double* __restrict__ corners_img,
                                                         int* __restrict__ counts) {
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  const double img_h = ori_shape[b * 2], img_w = ori_shape[b * 2 + 1];
  const double* cal = calib + (size_t)b * 6;
  const double rw = ratio[(size_t)b * ratio_pitch], rh = ratio[(size_t)b * ratio_pitch + 1];
  const double* ti = trans_inv ? trans_inv + (size_t)b * 6 : nullptr;  // read with undo_augment only (refused without it)
  const double* P = P2 ? P2 + (size_t)b * 12 : nullptr;
  double2* orow = (double2*)(rows + (size_t)b * R * 14);
  double2* oc3 = (double2*)(corners3d + (size_t)b * R * 24);
  double2* oci = corners_img ? (double2*)(corners_img + (size_t)b * R * 16) : nullptr;

  int start = 0, end = N;
  if (counts_in) {  // static layout; the entry has checked N == B * max_objs
    start = b * max_objs;
    end = start + min(max(counts_in[b], 0), max_objs);
  }
  const float fb = (float)b;
  int base = 0;
  for (int c0 = start; c0 < end; c0 += 64) {
    const int k = c0 + lane;
    const bool own = k < end && (counts_in != nullptr || in.batch_idx[k] == fb);
    const unsigned long long m = __ballot(own);
    const int j = base + __popcll(m & ((1ull << lane) - 1ull));
    if (own && j < R) {
      const int cid = (int)in.cls[k];
      const int cm = cid < 0 ? 0 : (cid >= nc ? nc - 1 : cid);
      const double bx = in.bboxes[(size_t)k * 4], by = in.bboxes[(size_t)k * 4 + 1];
      const double dw = in.bboxes[(size_t)k * 4 + 2] / 2, dh = in.bboxes[(size_t)k * 4 + 3] / 2;
      const double xu = bx * img_w;
      const double h = in.size_3d[(size_t)k * 3] + mean_size[cm * 3], w = in.size_3d[(size_t)k * 3 + 1] + mean_size[cm * 3 + 1],
                   l = in.size_3d[(size_t)k * 3 + 2] + mean_size[cm * 3 + 2];
      const double cx = in.center_3d[(size_t)k * 2], cy = in.center_3d[(size_t)k * 2 + 1];
      double u, v;
      if (undo_augment) {
        const double fx = (double)(float)cx, fy = (double)(float)cy;
        u = (ti[0] * fx + ti[1] * fy) + ti[2];
        v = (ti[3] * fx + ti[4] * fy) + ti[5];
      } else {
        u = cx / rw;
        v = cy / rh;
      }
      double lx, ly, lz;
      kitti_pixel_to_rect(u, v, in.depth[k], cal, use_camera_dis, lx, ly, lz);
      ly += h / 2;
      const double PI_D = 3.14159265358979323846;
      double alpha = (double)in.heading_bin[k] * (2 * PI_D / 12.0) + in.heading_res[k];  // decode_helper.py:3-10
      if (alpha > PI_D) alpha = alpha - 2 * PI_D;
      const double ry = kitti_alpha2ry(alpha, xu, cal[0], cal[2]);
      const double o[14] = {(double)cid, alpha, (bx - dw) * img_w, (by - dh) * img_h, (bx + dw) * img_w, (by + dh) * img_h, h, w, l, lx, ly,
                            lz, ry, 1.0};
#pragma unroll
      for (int i = 0; i < 7; ++i) orow[(size_t)j * 7 + i] = make_double2(o[2 * i], o[2 * i + 1]);
      double c3[24], ci[16];
      kitti_box_corners(h, w, l, lx, ly, lz, ry, P, c3, ci);
#pragma unroll
      for (int i = 0; i < 12; ++i) oc3[(size_t)j * 12 + i] = make_double2(c3[2 * i], c3[2 * i + 1]);
      if (oci && P) {
#pragma unroll
        for (int i = 0; i < 8; ++i) oci[(size_t)j * 8 + i] = make_double2(ci[2 * i], ci[2 * i + 1]);
      }
    }
    base += __popcll(m);
  }
  const int count = min(base, R);
  const double2 z = make_double2(0.0, 0.0);
  for (int j = count + lane; j < R; j += 64) {
#pragma unroll
    for (int i = 0; i < 7; ++i) orow[(size_t)j * 7 + i] = z;
#pragma unroll
    for (int i = 0; i < 12; ++i) oc3[(size_t)j * 12 + i] = z;
    if (oci) {
#pragma unroll
      for (int i = 0; i < 8; ++i) oci[(size_t)j * 8 + i] = z;
    }
  }
  if (lane == 0) counts[b] = count;
}

struct Span {
  const void* p;
  size_t bytes;
};

inline bool overlaps(const Span& a, const Span& b) {
  const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
  return a.p && b.p && a.bytes && b.bytes && a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

}  // namespace

extern "C" {

int y3d_decode_labels(const int64_t* cls, const double* bboxes, const double* center_3d, const double* size_3d, const double* depth,
                      const int64_t* heading_bin, const double* heading_res, const float* batch_idx, const int* counts_in, int N, int max_objs,
                      int B, const double* ori_shape, const double* calib, const double* ratio, int ratio_pitch, const double* trans_inv,
                      const double* P2, const double* mean_size, int nc, int use_camera_dis, int undo_augment, int R, double* rows,
                      double* corners3d, double* corners_img, int* counts, void* stream) {
  Y3D_CHECK(B >= 1 && N >= 0 && nc >= 1, "decode_labels: bad sizes (B = %d, N = %d, nc = %d)", B, N, nc);
  Y3D_CHECK(R >= 1, "decode_labels: R = %d (at least one slot per image)", R);
  Y3D_CHECK(rows && corners3d && counts, "decode_labels: null output");
  Y3D_CHECK((P2 != nullptr) == (corners_img != nullptr), "decode_labels: corners_img goes with P2 (both or neither)");
  Y3D_CHECK((((uintptr_t)rows | (uintptr_t)corners3d | (uintptr_t)corners_img) & 15) == 0 && ((uintptr_t)counts & 3) == 0,
            "decode_labels: rows, corners3d and corners_img must be 16-byte aligned, counts 4-byte aligned");
  Y3D_CHECK(ori_shape && calib && ratio && mean_size, "decode_labels: null per-image argument");
  Y3D_CHECK(ratio_pitch == 2 || ratio_pitch == 4, "decode_labels: ratio_pitch %d (2: (B, 2), 4: (B, 2, 2))", ratio_pitch);
  Y3D_CHECK(!undo_augment || trans_inv, "decode_labels: undo_augment needs trans_inv");
  Y3D_CHECK(N == 0 || (cls && bboxes && center_3d && size_3d && depth && heading_bin && heading_res), "decode_labels: null per-box argument");
  if (counts_in) {
    Y3D_CHECK(max_objs >= 1 && (long)N == (long)B * max_objs, "decode_labels: static layout of %d rows, expected B * max_objs = %d * %d", N, B,
              max_objs);
  } else {
    Y3D_CHECK(N == 0 || batch_idx, "decode_labels: the ragged layout needs batch_idx");
  }
  // byte ranges, so that an output overlapping an input at an offset (views into one allocation) is caught too
  const size_t n = (size_t)N, br = (size_t)B * R;
  const Span ins[] = {{cls, n * 8},         {bboxes, n * 32},      {center_3d, n * 16},       {size_3d, n * 24},
                      {depth, n * 8},       {heading_bin, n * 8},  {heading_res, n * 8},      {batch_idx, counts_in ? 0 : n * 4},
                      {counts_in, (size_t)B * 4}, {ori_shape, (size_t)B * 16}, {calib, (size_t)B * 48}, {ratio, (size_t)B * ratio_pitch * 8},
                      {trans_inv, (size_t)B * 48}, {P2, (size_t)B * 96}, {mean_size, (size_t)nc * 24}};
  const Span outs[] = {{rows, br * 14 * 8}, {corners3d, br * 24 * 8}, {corners_img, br * 16 * 8}, {counts, (size_t)B * 4}};
  for (int o = 0; o < 4; ++o) {
    for (const Span& i : ins) Y3D_CHECK(!overlaps(outs[o], i), "decode_labels: an output overlaps an input");
    for (int q = o + 1; q < 4; ++q) Y3D_CHECK(!overlaps(outs[o], outs[q]), "decode_labels: the outputs overlap each other");
  }
  const LabelIn in{cls, bboxes, center_3d, size_3d, depth, heading_bin, heading_res, batch_idx};
  hipLaunchKernelGGL(decode_labels_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, in, counts_in, N, max_objs, ori_shape, calib, ratio,
                     ratio_pitch, trans_inv, P2, mean_size, nc, use_camera_dis, undo_augment, R, rows, corners3d, corners_img, counts);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

}  // extern "C"
