// Validator box metrics on the device: precision, recall, mAP50 and mAP50-95 over ten IoU thresholds (paths relative to ultralytics/):
//   * box_iou                                   utils/metrics.py:53 (fp32, (area1 + area2 - inter) + eps in that order)
//   * match_predictions, use_scipy = False      engine/validator.py:229-273, iouv = linspace(0.5, 0.95, 10) (models/yolo/detect/val.py:40)
//   * the validators' box preparation           models/yolo/detect/val.py:97-175 (_prepare_batch / _prepare_pred: xywh2xyxy * imgsz,
//                                               scale_boxes utils/ops.py:89, clip_boxes :306); models/yolov10_3D/val.py:114-187
//                                               (decode_preds_eval rows; decode_batch_eval targets, data/datasets/kitti.py:466-512)
//   * ap_per_class / compute_ap                 utils/metrics.py:532, :499 (per-class cumulative counts, fp64 recall / precision, the
//                                               precision envelope, np.interp at the 101- and 1000-point grids, np.trapz)
//
// Matching.  The two np.unique steps of match_predictions amount to: L(d) = d's class-matched label with the largest IoU, m(d) that IoU;
// d is a true positive at threshold t iff m(d) >= t and no d' < d has L(d') = L(d) with m(d') >= t (the first unique keeps each
// detection's best label and re-orders by detection index, so the second gives a label to its lowest-index claimant, which does not
// fall back to its second-best label).  Claims are an atomicMin of the detection index into a per-(gt, threshold) LDS table.
// Deliberate tie rules where the reference is implementation-defined (its argsort is an unstable quicksort): an IoU tie between two
// labels of one detection goes to the higher gt index (what a stable sort, reversed, gives); confidence ties keep accumulation order.
//
// np.interp(x, xp, fp, left, right), restated: j = the LAST index with xp[j] <= x; x < xp[0] -> left, x > xp[-1] -> right; x == xp[j]
// or j the last index -> fp[j]; otherwise slope * (x - xp[j]) + fp[j], slope = (fp[j+1] - fp[j]) / (xp[j+1] - xp[j]).  Each grid point
// has exactly one owning sample j, so the kernels write every point once: a sample owns the grid points in [xp[j], xp[j+1]).
//
// Confusion matrix.  ConfusionMatrix.process_batch (utils/metrics.py:319-376), fed per image by both validators' update_metrics
// (models/yolo/detect/val.py:137, :151; models/yolov10_3D/val.py:138, :156).  Boxes and IoUs are the matcher's own (the same device
// functions), so every IoU is bit for bit the one behind the tp masks.  A detection takes part iff its row is kept and conf_row > conf
// (strict, in the row's precision: fp32 for 2D rows, fp64 for 3D rows); candidate pairs are those with iou > (float)iou_thres (strict),
// whatever their classes.  The two np.unique steps amount to two argmax passes: each detection keeps its best gt, then each gt keeps the
// best of the detections that chose it; a detection that loses does not fall back to its second-best gt.  Both passes are LDS claims
// (atomicMax of the IoU bits, then of the detection index among the holders of that maximum).  Counting: a matched gt i with detection
// d -> matrix[cls(d), cls(i)]; an unmatched gt -> matrix[nc, cls(i)]; when the image has at least one match, every participating
// detection left unmatched -> matrix[cls(d), nc].  When the image has NO match its detections add nothing: that is the reference's
// `if n:` guard (:373) and is kept on purpose.  An image with gts and no rows (the validators' `detections=None` call) counts every gt
// as missed, as does one whose rows all fail the filter.  An image WITHOUT gts: the batched entry adds nothing, because neither
// validator calls process_batch for it (`if nl:`); the single-image entry behind the drop-in counts matrix[cls(d), nc] for every
// participating detection (:330-336).  single_cls zeroes the detection class only, as both validators do.
// Deliberate tie rules where the reference is implementation-defined (argsort()[::-1] of an unstable sort) - what a stable sort,
// reversed, gives: an IoU tie between two gts of one detection goes to the higher gt index; an IoU tie between two detections that chose
// one gt goes to the higher detection index.
// All writes to the matrix are integer atomicAdds, so two runs give identical matrices.  status[0]: atomicMax of the gt count of an
// image above DM_MAX_GT (that image adds nothing); status[1]: set when a class outside [0, nc) was met (the reference raises IndexError;
// such a box is not counted).
//
// Limits: DM_MAX_GT gts and DM_MAX_DET detections per image, DM_MAX_THR thresholds.  No kernel uses scratch (all run-time indexed
// state is in LDS).
#include "common.h"

#include <climits>

#pragma clang fp contract(off)

namespace {

constexpr int DM_MAX_GT = 512;
constexpr int DM_MAX_DET = 1024;
constexpr int DM_MAX_THR = 16;
constexpr int DM_BLOCK = 256;
constexpr int DM_MAX_AP_PTS = 129;     // np.trapz's add.reduce: one pairwise block (<= 128 terms)
constexpr int DM_MAX_CURVE_PTS = 1024;

enum { MODE_2D = 0, MODE_3D = 1, MODE_IOU = 2, MODE_XYXY = 3 };

// box_iou (utils/metrics.py:53-75) for one pair, a = gt, b = det, fp32 in the reference's operation order
__device__ __forceinline__ float pair_iou(float a1x, float a1y, float a2x, float a2y, float b1x, float b1y, float b2x, float b2y, float eps) {
  const float iw = fmaxf(fminf(a2x, b2x) - fmaxf(a1x, b1x), 0.f);
  const float ih = fmaxf(fminf(a2y, b2y) - fmaxf(a1y, b1y), 0.f);
  const float inter = iw * ih;
  const float area1 = (a2x - a1x) * (a2y - a1y);
  const float area2 = (b2x - b1x) * (b2y - b1y);
  return inter / (((area1 + area2) - inter) + eps);
}

// inclusive block scan (sum) of one int per lane over DM_BLOCK lanes; s must hold DM_BLOCK ints; `reverse` scans from the high lane down
template <bool reverse>
__device__ int block_scan_sum(int v, int* s) {
  const int tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (int off = 1; off < DM_BLOCK; off <<= 1) {
    const int o = reverse ? tid + off : tid - off;
    const int add = (o >= 0 && o < DM_BLOCK) ? s[o] : 0;
    __syncthreads();
    s[tid] += add;
    __syncthreads();
  }
  return s[tid];
}

// inclusive suffix max of one double per lane
__device__ double block_suffix_max(double v, double* s) {
  const int tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (int off = 1; off < DM_BLOCK; off <<= 1) {
    const double o = tid + off < DM_BLOCK ? s[tid + off] : 0.0;
    __syncthreads();
    s[tid] = fmax(s[tid], o);
    __syncthreads();
  }
  return s[tid];
}

// The image's gts in batch order (ordered compaction of batch_idx == b), prepared as _prepare_batch / decode_batch_eval do; shared by
// the matcher and the confusion kernel.  P has meta, gt_img, gt_cls, gt_box, n_gt, img_h, img_w.  Returns the image's gt count, which
// may exceed DM_MAX_GT: only the first DM_MAX_GT are stored.  Every lane of the workgroup must call it.
template <int MODE, class P>
__device__ __forceinline__ int load_gts(const P& p, int b, float (*s_gb)[4], int* s_gc, int* s_scan) {
  const int tid = threadIdx.x;
  int ng = 0;
  float h0 = 0.f, w0 = 0.f, gain = 1.f, padw = 0.f, padh = 0.f;
  if (MODE == MODE_2D) {
    const double* m = p.meta + (size_t)b * 5;
    h0 = (float)m[0]; w0 = (float)m[1]; gain = (float)m[2]; padw = (float)m[3]; padh = (float)m[4];
  } else {
    h0 = (float)p.meta[(size_t)b * 2]; w0 = (float)p.meta[(size_t)b * 2 + 1];
  }
  for (int base = 0; base < p.n_gt; base += DM_BLOCK) {
    const int i = base + tid;
    const int f = (i < p.n_gt && p.gt_img[i] == (float)b) ? 1 : 0;
    const int incl = block_scan_sum<false>(f, s_scan);
    const int pos = ng + incl - f;
    if (f && pos < DM_MAX_GT) {
      const float* q = p.gt_box + (size_t)i * 4;
      const float dw = q[2] / 2.f, dh = q[3] / 2.f;
      float x1 = q[0] - dw, y1 = q[1] - dh, x2 = q[0] + dw, y2 = q[1] + dh;
      if (MODE == MODE_2D) {  // xywh2xyxy(bbox) * imgsz[[1, 0, 1, 0]], then scale_boxes: - pad, / gain, clip to ori_shape
        const float W = (float)p.img_w, H = (float)p.img_h;
        x1 = x1 * W; y1 = y1 * H; x2 = x2 * W; y2 = y2 * H;
        x1 = (x1 - padw) / gain; y1 = (y1 - padh) / gain; x2 = (x2 - padw) / gain; y2 = (y2 - padh) / gain;
        x1 = fminf(fmaxf(x1, 0.f), w0); y1 = fminf(fmaxf(y1, 0.f), h0); x2 = fminf(fmaxf(x2, 0.f), w0); y2 = fminf(fmaxf(y2, 0.f), h0);
      } else {                // xywh2xyxy(bbox) * ori_shape[[1, 0, 1, 0]]; exact in the reference's fp64, rounded once by box_iou
        x1 = x1 * w0; y1 = y1 * h0; x2 = x2 * w0; y2 = y2 * h0;
      }
      s_gb[pos][0] = x1; s_gb[pos][1] = y1; s_gb[pos][2] = x2; s_gb[pos][3] = y2;
      s_gc[pos] = (int)p.gt_cls[i];
    }
    ng += s_scan[DM_BLOCK - 1];
    __syncthreads();
  }
  return ng;
}

// Row r = b * K + k of a batched mode as the validators prepare it: the fp32 xyxy box box_iou sees and the class (0 under single_cls)
template <int MODE, class P>
__device__ __forceinline__ void prep_det(const P& p, int b, size_t r, float& x1, float& y1, float& x2, float& y2, int& c) {
  if (MODE == MODE_2D) {  // _prepare_pred: scale_boxes on a clone of the row
    const float* q = (const float*)p.preds + r * 6;
    const double* mt = p.meta + (size_t)b * 5;
    const float h0 = (float)mt[0], w0 = (float)mt[1], gain = (float)mt[2], padw = (float)mt[3], padh = (float)mt[4];
    x1 = (q[0] - padw) / gain; y1 = (q[1] - padh) / gain; x2 = (q[2] - padw) / gain; y2 = (q[3] - padh) / gain;
    x1 = fminf(fmaxf(x1, 0.f), w0); y1 = fminf(fmaxf(y1, 0.f), h0); x2 = fminf(fmaxf(x2, 0.f), w0); y2 = fminf(fmaxf(y2, 0.f), h0);
    c = p.single_cls ? 0 : (int)q[5];
  } else {                // decode row: box cols 2:6 (fp64, cast by box_iou), class col 0
    const double* q = (const double*)p.preds + r * 14;
    x1 = (float)q[2]; y1 = (float)q[3]; x2 = (float)q[4]; y2 = (float)q[5];
    c = p.single_cls ? 0 : (int)q[0];
  }
}

struct MatchP {
  const void* preds;          // MODE_2D (B, K, 6) f32 | MODE_3D (B, K, 14) f64 | MODE_IOU (n_gt, K) f32 IoU matrix
  const unsigned char* keep;  // (B, K) or NULL
  const double* meta;         // MODE_2D (B, 5) [h0, w0, gain, padw, padh]; MODE_3D (B, 2) [h0, w0]
  const float* gt_img;        // (n_gt) image index of each gt (float as collated), NULL in MODE_IOU
  const float* gt_cls;        // (n_gt) class (float as collated), MODE_IOU: NULL (int classes below)
  const int* gt_cls_i;        // MODE_IOU: (n_gt) int32 classes
  const int* det_cls_i;       // MODE_IOU: (K) int32 classes
  const float* gt_box;        // (n_gt, 4) xywh, normalised
  const float* thr;           // (n_thr) fp32 IoU thresholds, > 0
  int B, K, n_gt, n_thr, img_h, img_w, single_cls;
  float eps;
  int* tp;                    // out: bit t = correct at thr[t]
  double* conf;               // out (batched modes): the detection's confidence, or 0
  int* cls;                   // out (batched modes): the detection's class, -1 where the row is not a detection
  int* status;                // out (batched modes): atomicMax'd with the gt count of an image above DM_MAX_GT
};

template <int MODE>
__global__ void __launch_bounds__(DM_BLOCK) box_match_kernel(MatchP p) {
  __shared__ float s_gb[DM_MAX_GT][4];
  __shared__ int s_gc[DM_MAX_GT];
  __shared__ int s_claim[DM_MAX_GT * DM_MAX_THR];
  __shared__ int s_best[DM_MAX_DET];
  __shared__ float s_m[DM_MAX_DET];
  __shared__ int s_scan[DM_BLOCK];
  const int tid = threadIdx.x, b = blockIdx.x, K = p.K, nthr = p.n_thr;

  // 1. the image's gts in batch order (ordered compaction of batch_idx == b), prepared as _prepare_batch / decode_batch_eval do
  int ng = 0;
  if (MODE == MODE_IOU) {
    ng = p.n_gt;  // host-checked <= DM_MAX_GT
    for (int g = tid; g < ng; g += DM_BLOCK) s_gc[g] = p.gt_cls_i[g];
  } else {
    ng = load_gts<MODE>(p, b, s_gb, s_gc, s_scan);
    if (ng > DM_MAX_GT) {  // refused: get_stats raises; never index past the tables
      if (tid == 0) atomicMax(p.status, ng);
      ng = 0;
    }
  }
  for (int j = tid; j < ng * nthr; j += DM_BLOCK) s_claim[j] = INT_MAX;
  __syncthreads();

  // 2. each detection's best class-matched label (ties -> the higher gt index) and its claims
  for (int k = tid; k < K; k += DM_BLOCK) {
    const size_t r = (size_t)b * K + k;
    const bool valid = MODE == MODE_IOU || p.keep == nullptr || p.keep[r] != 0;
    int best = -1;
    float m = 0.f;
    if (valid) {
      if (MODE == MODE_IOU) {
        const float* iou = (const float*)p.preds;
        const int c = p.det_cls_i[k];
        for (int g = 0; g < ng; ++g) {
          if (s_gc[g] != c) continue;
          const float v = iou[(size_t)g * K + k];
          if (v >= m) { m = v; best = g; }
        }
      } else {
        float x1, y1, x2, y2;
        int c;
        prep_det<MODE>(p, b, r, x1, y1, x2, y2, c);
        for (int g = 0; g < ng; ++g) {
          if (s_gc[g] != c) continue;
          const float v = pair_iou(s_gb[g][0], s_gb[g][1], s_gb[g][2], s_gb[g][3], x1, y1, x2, y2, p.eps);
          if (v >= m) { m = v; best = g; }
        }
      }
      if (best >= 0)
        for (int t = 0; t < nthr; ++t)
          if (m >= p.thr[t]) atomicMin(&s_claim[best * nthr + t], k);
    }
    s_best[k] = best;
    s_m[k] = m;
  }
  __syncthreads();

  // 3. true-positive masks (+ confidence and class of the batched modes), one slot per row
  for (int k = tid; k < K; k += DM_BLOCK) {
    const size_t r = (size_t)b * K + k;
    const int best = s_best[k];
    int mask = 0;
    if (best >= 0)
      for (int t = 0; t < nthr; ++t)
        if (s_m[k] >= p.thr[t] && s_claim[best * nthr + t] == k) mask |= 1 << t;
    p.tp[r] = mask;
    if (MODE != MODE_IOU) {
      const bool valid = p.keep == nullptr || p.keep[r] != 0;
      double cf = 0.0;
      int c = -1;
      if (valid) {
        if (MODE == MODE_2D) {
          const float* q = (const float*)p.preds + r * 6;
          cf = (double)q[4];
          c = p.single_cls ? 0 : (int)q[5];
        } else {
          const double* q = (const double*)p.preds + r * 14;
          cf = q[13];
          c = p.single_cls ? 0 : (int)q[0];
        }
      }
      p.conf[r] = cf;
      p.cls[r] = c;
    }
  }
}

struct ConfP {
  const void* preds;          // MODE_2D (B, K, 6) f32 | MODE_3D (B, K, 14) f64 | MODE_XYXY (K, 6) f32 or f64 (det_f64), NULL with K = 0
  const unsigned char* keep;  // (B, K) or NULL
  const double* meta;         // as MatchP (NULL in MODE_XYXY)
  const float* gt_img;        // (n_gt), NULL in MODE_XYXY
  const float* gt_cls;        // (n_gt) float as collated, NULL in MODE_XYXY
  const int* gt_cls_i;        // MODE_XYXY: (n_gt) int32 classes
  const float* gt_box;        // (n_gt, 4): normalised xywh | MODE_XYXY: prepared xyxy
  int B, K, n_gt, img_h, img_w, single_cls, nc, det_f64;
  int count_empty;            // an image without gts counts its detections as false positives (the drop-in; the validators skip it)
  float eps, iou_thres;
  double conf;
  int* matrix;                // (nc + 1, nc + 1), added into
  int* status;                // [0] atomicMax'd with the gt count of an image above DM_MAX_GT, [1] set by a class outside [0, nc)
};

// One workgroup per image; the rules are in the file header.
template <int MODE>
__global__ void __launch_bounds__(DM_BLOCK) confusion_kernel(ConfP p) {
  __shared__ float s_gb[DM_MAX_GT][4];
  __shared__ int s_gc[DM_MAX_GT];
  __shared__ unsigned s_gmax[DM_MAX_GT];  // the bits of the largest IoU among the detections that chose the gt (IoUs here are > 0)
  __shared__ int s_gdet[DM_MAX_GT];       // the gt's detection, -1 = unmatched
  __shared__ int s_best[DM_MAX_DET];      // the detection's gt, -1 = none above the threshold, -2 = the row takes no part
  __shared__ float s_m[DM_MAX_DET];
  __shared__ int s_dc[DM_MAX_DET];
  __shared__ int s_scan[DM_BLOCK];
  __shared__ int s_any;
  const int tid = threadIdx.x, b = blockIdx.x, K = p.K, nc = p.nc, ld = p.nc + 1;

  // 1. the image's gts, exactly the matcher's
  int ng;
  if (MODE == MODE_XYXY) {
    ng = p.n_gt;  // host-checked <= DM_MAX_GT
    for (int g = tid; g < ng; g += DM_BLOCK) {
      const float* q = p.gt_box + (size_t)g * 4;
      s_gb[g][0] = q[0]; s_gb[g][1] = q[1]; s_gb[g][2] = q[2]; s_gb[g][3] = q[3];
      s_gc[g] = p.gt_cls_i[g];
    }
  } else {
    ng = load_gts<MODE>(p, b, s_gb, s_gc, s_scan);
    if (ng > DM_MAX_GT) {  // refused: the image adds nothing and reading the matrix raises; never index past the tables
      if (tid == 0) atomicMax(p.status, ng);
      return;
    }
  }
  if (ng == 0 && !p.count_empty) return;  // neither validator calls process_batch for an image without gts
  for (int g = tid; g < ng; g += DM_BLOCK) { s_gmax[g] = 0u; s_gdet[g] = -1; }
  if (tid == 0) s_any = ng == 0 ? 1 : 0;  // utils/metrics.py:330-336 counts every detection of an image without gts
  __syncthreads();

  // 2. each participating detection's best gt above the threshold, whatever the classes (ties -> the higher gt index), and the
  //    largest IoU among each gt's claimants
  for (int k = tid; k < K; k += DM_BLOCK) {
    const size_t r = (size_t)b * K + k;
    bool part = MODE == MODE_XYXY || p.keep == nullptr || p.keep[r] != 0;
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
    int c = 0;
    if (part) {
      if (MODE == MODE_XYXY) {
        if (p.det_f64) {
          const double* q = (const double*)p.preds + r * 6;
          x1 = (float)q[0]; y1 = (float)q[1]; x2 = (float)q[2]; y2 = (float)q[3];
          part = q[4] > p.conf;
          c = (int)q[5];
        } else {
          const float* q = (const float*)p.preds + r * 6;
          x1 = q[0]; y1 = q[1]; x2 = q[2]; y2 = q[3];
          part = q[4] > (float)p.conf;
          c = (int)q[5];
        }
      } else {
        prep_det<MODE>(p, b, r, x1, y1, x2, y2, c);
        if (MODE == MODE_2D) part = ((const float*)p.preds)[r * 6 + 4] > (float)p.conf;
        else part = ((const double*)p.preds)[r * 14 + 13] > p.conf;
      }
      if (part && (c < 0 || c >= nc)) {
        p.status[1] = 1;
        part = false;
      }
    }
    int best = -1;
    float m = 0.f;
    if (part) {
      for (int g = 0; g < ng; ++g) {
        const float v = pair_iou(s_gb[g][0], s_gb[g][1], s_gb[g][2], s_gb[g][3], x1, y1, x2, y2, p.eps);
        if (v > p.iou_thres && v >= m) { m = v; best = g; }
      }
      if (best >= 0) {
        atomicMax(&s_gmax[best], __float_as_uint(m));
        s_any = 1;
      }
    }
    s_best[k] = part ? best : -2;
    s_m[k] = m;
    s_dc[k] = c;
  }
  __syncthreads();

  // 3. each gt keeps the best of the detections that chose it (ties -> the higher detection index)
  for (int k = tid; k < K; k += DM_BLOCK) {
    const int best = s_best[k];
    if (best >= 0 && __float_as_uint(s_m[k]) == s_gmax[best]) atomicMax(&s_gdet[best], k);
  }
  __syncthreads();

  // 4. counts
  for (int g = tid; g < ng; g += DM_BLOCK) {
    const int gc = s_gc[g], d = s_gdet[g];
    if (gc < 0 || gc >= nc) {
      p.status[1] = 1;
      continue;
    }
    atomicAdd(&p.matrix[(d >= 0 ? s_dc[d] : nc) * ld + gc], 1);
  }
  if (s_any)  // the reference's `if n:` guard: without a single match in the image its detections are not counted
    for (int k = tid; k < K; k += DM_BLOCK) {
      const int best = s_best[k];
      if (best == -2 || (best >= 0 && s_gdet[best] == k)) continue;
      atomicAdd(&p.matrix[s_dc[k] * ld + nc], 1);
    }
}

__global__ void box_iou_kernel(const float* a, int na, const float* bx, int nb, float eps, float* out) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)na * nb) return;
  const int i = (int)(idx / nb), j = (int)(idx % nb);
  const float* A = a + (size_t)i * 4;
  const float* Bq = bx + (size_t)j * 4;
  out[idx] = pair_iou(A[0], A[1], A[2], A[3], Bq[0], Bq[1], Bq[2], Bq[3], eps);
}

// first index k of x[0..n) with x[k] >= v (ge) or x[k] > v (!ge); x ascending
template <bool ge>
__device__ __forceinline__ int grid_bound(const double* x, int n, double v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ge ? (x[mid] < v) : (x[mid] <= v)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

struct ApP {
  const int* tp;        // (n) sorted by (class, confidence descending)
  const double* conf;
  const int* cls;
  long n;
  const int* ucls;      // (nc) classes with targets
  const double* nl;     // (nc) n_l + eps
  int n_thr;
  const double* x_ap;   // (n_ap) np.linspace(0, 1, 101)
  int n_ap;
  const double* x_cv;   // (n_cv) np.linspace(0, 1, 1000)
  int n_cv;
  double* ap;           // (nc, n_thr)
  double* p_curve;      // (nc, n_cv)
  double* r_curve;
};

// One workgroup per (class, threshold).  One pass from the last detection of the class down to the first: tpc[i] = total - (true
// positives after i), so recall, precision and the envelope (a suffix max) are all known when sample i is reached, and each sample
// writes the grid points it owns.  The threshold-0 workgroup also writes the class's 1000-point recall / precision curves.
__global__ void __launch_bounds__(DM_BLOCK) ap_kernel(ApP p) {
  __shared__ double s_xap[DM_MAX_AP_PTS];
  __shared__ double s_xcv[DM_MAX_CURVE_PTS];
  __shared__ double s_y[DM_MAX_AP_PTS];
  __shared__ int s_scan[DM_BLOCK];
  __shared__ double s_dscan[DM_BLOCK];
  __shared__ double s_r[DM_BLOCK], s_env[DM_BLOCK], s_p[DM_BLOCK], s_cf[DM_BLOCK];
  __shared__ int s_kap[DM_BLOCK], s_kcv[DM_BLOCK];
  __shared__ long s_lo, s_hi;
  __shared__ int s_total;
  const int tid = threadIdx.x, c = blockIdx.x, t = blockIdx.y;
  const bool curves = t == 0;
  for (int k = tid; k < p.n_ap; k += DM_BLOCK) s_xap[k] = p.x_ap[k];
  if (curves)
    for (int k = tid; k < p.n_cv; k += DM_BLOCK) s_xcv[k] = p.x_cv[k];
  if (tid == 0) {
    const int cc = p.ucls[c];
    long lo = 0, hi = p.n;
    while (lo < hi) { const long mid = (lo + hi) >> 1; if (p.cls[mid] < cc) lo = mid + 1; else hi = mid; }
    long e = lo, h2 = p.n;
    while (e < h2) { const long mid = (e + h2) >> 1; if (p.cls[mid] <= cc) e = mid + 1; else h2 = mid; }
    s_lo = lo;
    s_hi = e;
  }
  __syncthreads();
  const long lo = s_lo, n = s_hi - s_lo;
  double* pc = p.p_curve + (size_t)c * p.n_cv;
  double* rc = p.r_curve + (size_t)c * p.n_cv;
  if (n == 0) {  // targets but no detections: AP 0, zero curves (the reference's `continue`)
    if (tid == 0) p.ap[(size_t)c * p.n_thr + t] = 0.0;
    if (curves)
      for (int k = tid; k < p.n_cv; k += DM_BLOCK) { pc[k] = 0.0; rc[k] = 0.0; }
    return;
  }
  const double nl = p.nl[c];

  int cnt = 0;
  for (long i = tid; i < n; i += DM_BLOCK) cnt += (p.tp[lo + i] >> t) & 1;
  cnt = block_scan_sum<false>(cnt, s_scan);
  if (tid == DM_BLOCK - 1) s_total = cnt;
  __syncthreads();
  const int total = s_total;

  // carries from the chunk above (higher indices); above the last sample sit the sentinels mrec = 1, mpre = 0
  int carry_cnt = 0;
  double nxt_r = 1.0, nxt_env = 0.0, nxt_p = 0.0, nxt_cf = 0.0;
  const int k_one = grid_bound<true>(s_xap, p.n_ap, 1.0);
  int nxt_kap = k_one, nxt_kcv = 0;
  for (int k = k_one + tid; k < p.n_ap; k += DM_BLOCK) s_y[k] = 0.0;  // x >= 1: the last sentinel, mpre = 0
  for (long end = n; end > 0; end -= DM_BLOCK) {
    const long i = end - DM_BLOCK + tid;
    const bool v = i >= 0;
    const int bit = v ? (p.tp[lo + i] >> t) & 1 : 0;
    const int suf = block_scan_sum<true>(bit, s_scan);           // true positives in [i, end); s_scan keeps them
    const int tpc = total - carry_cnt - suf + bit;                // true positives in [0, i]
    const double r = (double)tpc / nl;
    const double pr = v ? (double)tpc / (double)(i + 1) : 0.0;
    const double env = fmax(block_suffix_max(pr, s_dscan), nxt_env);
    const double cf = v ? p.conf[lo + i] : 0.0;
    const int kap = v ? grid_bound<true>(s_xap, p.n_ap, r) : 0;                 // first 101-grid point >= recall
    const int kcv = (v && curves) ? grid_bound<false>(s_xcv, p.n_cv, cf) : 0;  // first 1000-grid point > confidence
    s_r[tid] = r; s_env[tid] = env; s_p[tid] = pr; s_cf[tid] = cf;
    s_kap[tid] = kap; s_kcv[tid] = kcv;
    __syncthreads();
    const bool top = tid == DM_BLOCK - 1;  // its neighbour i + 1 is in the chunk above (or is the sentinel)
    const double r1 = top ? nxt_r : s_r[tid + 1];
    const double env1 = top ? nxt_env : s_env[tid + 1];
    const int kap1 = top ? nxt_kap : s_kap[tid + 1];
    if (v) {
      // 101-point grid: mrec index i + 1 owns x in [recall_i, recall_{i+1})
      for (int k = kap; k < kap1; ++k) {
        const double x = s_xap[k];
        s_y[k] = x == r ? env : (env1 - env) / (r1 - r) * (x - r) + env;
      }
      if (curves) {  // xp = -conf (ascending), query -x: sample i owns x in (conf_{i+1}, conf_i], the last sample also x <= conf_{n-1}
        const bool last = i == n - 1;
        const double p1 = top ? nxt_p : s_p[tid + 1];
        const double cf1 = top ? nxt_cf : s_cf[tid + 1];
        const int k0 = last ? 0 : (top ? nxt_kcv : s_kcv[tid + 1]);
        const double xpj = -cf;
        for (int k = k0; k < kcv; ++k) {
          const double q = -s_xcv[k];
          if (last || q == xpj) {
            rc[k] = r;
            pc[k] = pr;
          } else {
            const double dx = -cf1 - xpj;
            rc[k] = (r1 - r) / dx * (q - xpj) + r;
            pc[k] = (p1 - pr) / dx * (q - xpj) + pr;
          }
        }
        if (i == 0)
          for (int k = kcv; k < p.n_cv; ++k) { rc[k] = 0.0; pc[k] = 1.0; }  // x > conf_0: left = 0 / 1
      }
    }
    // carries for the chunk below: its neighbour is this chunk's lowest valid lane
    const int first = end < DM_BLOCK ? (int)(DM_BLOCK - end) : 0;
    carry_cnt += s_scan[first];
    nxt_r = s_r[first]; nxt_env = s_env[first]; nxt_p = s_p[first]; nxt_cf = s_cf[first];
    nxt_kap = s_kap[first]; nxt_kcv = s_kcv[first];
    __syncthreads();
  }
  // the first sentinel: mrec = 0, mpre = max(1, envelope) owns x in [0, recall_0)
  if (tid == 0) {
    const double env0 = fmax(1.0, nxt_env);
    for (int k = grid_bound<true>(s_xap, p.n_ap, 0.0); k < nxt_kap; ++k) {
      const double x = s_xap[k];
      s_y[k] = x == 0.0 ? env0 : (nxt_env - env0) / (nxt_r - 0.0) * (x - 0.0) + env0;
    }
  }
  __syncthreads();
  // np.trapz: add.reduce(d * (y[1:] + y[:-1]) / 2.0) from 0.0, numpy's pairwise order for <= 128 terms (8 accumulators, then the rest)
  if (tid == 0) {
    const int m = p.n_ap - 1;
    double acc = 0.0;
    if (m < 8) {
      for (int k = 0; k < m; ++k) acc += (s_xap[k + 1] - s_xap[k]) * (s_y[k + 1] + s_y[k]) / 2.0;
    } else {
      double a[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = (s_xap[j + 1] - s_xap[j]) * (s_y[j + 1] + s_y[j]) / 2.0;
      int k = 8;
      for (; k < m - (m % 8); k += 8)
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] += (s_xap[k + j + 1] - s_xap[k + j]) * (s_y[k + j + 1] + s_y[k + j]) / 2.0;
      acc = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
      for (; k < m; ++k) acc += (s_xap[k + 1] - s_xap[k]) * (s_y[k + 1] + s_y[k]) / 2.0;
    }
    p.ap[(size_t)c * p.n_thr + t] = 0.0 + acc;
  }
}

}  // namespace

extern "C" {

int y3d_det_metrics_max_gts(void) { return DM_MAX_GT; }
int y3d_det_metrics_max_dets(void) { return DM_MAX_DET; }

int y3d_box_iou(const float* box1, int n1, const float* box2, int n2, float eps, float* out, void* stream) {
  Y3D_CHECK(n1 >= 0 && n2 >= 0 && (n1 == 0 || n2 == 0 || (box1 && box2 && out)), "box_iou: bad arguments");
  const long total = (long)n1 * n2;
  if (total == 0) return Y3D_OK;
  hipLaunchKernelGGL(box_iou_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, box1, n1, box2, n2, eps, out);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

static int match_args(const char* who, int K, int n_thr, const float* thr, const int* tp) {
  Y3D_CHECK(K >= 0 && K <= DM_MAX_DET, "%s: %d detections per image (at most %d)", who, K, DM_MAX_DET);
  Y3D_CHECK(n_thr >= 1 && n_thr <= DM_MAX_THR && thr && tp, "%s: %d thresholds (1 .. %d)", who, n_thr, DM_MAX_THR);
  return Y3D_OK;
}

int y3d_match_predictions(const float* iou, const int* gt_cls, int n_gt, const int* det_cls, int n_det, const float* thr, int n_thr,
                          int* tp, void* stream) {
  if (match_args("match_predictions", n_det, n_thr, thr, tp)) return Y3D_ERR_INVALID;
  Y3D_CHECK(n_gt >= 0 && n_gt <= DM_MAX_GT, "match_predictions: %d labels (at most %d)", n_gt, DM_MAX_GT);
  Y3D_CHECK(n_gt == 0 || (iou && gt_cls && det_cls), "match_predictions: null argument");
  if (n_det == 0) return Y3D_OK;
  MatchP p{};
  p.preds = iou; p.gt_cls_i = gt_cls; p.det_cls_i = det_cls; p.thr = thr;
  p.B = 1; p.K = n_det; p.n_gt = n_gt; p.n_thr = n_thr; p.tp = tp;
  hipLaunchKernelGGL(box_match_kernel<MODE_IOU>, dim3(1), dim3(DM_BLOCK), 0, (hipStream_t)stream, p);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_box_match_batch(int mode, const void* preds, const unsigned char* keep, int B, int K, const double* meta, int img_h, int img_w,
                        int single_cls, const float* gt_img, const float* gt_cls, const float* gt_box, int n_gt, const float* thr,
                        int n_thr, int* tp, double* conf, int* cls, int* status, void* stream) {
  if (match_args("box_match_batch", K, n_thr, thr, tp)) return Y3D_ERR_INVALID;
  Y3D_CHECK(mode == MODE_2D || mode == MODE_3D, "box_match_batch: mode must be 0 (2D) or 1 (3D), got %d", mode);
  Y3D_CHECK(B >= 0 && n_gt >= 0 && preds && meta && conf && cls && status, "box_match_batch: bad arguments");
  Y3D_CHECK(n_gt == 0 || (gt_img && gt_cls && gt_box), "box_match_batch: null gt arrays");
  if (B == 0 || K == 0) return Y3D_OK;
  MatchP p{};
  p.preds = preds; p.keep = keep; p.meta = meta; p.gt_img = gt_img; p.gt_cls = gt_cls; p.gt_box = gt_box; p.thr = thr;
  p.B = B; p.K = K; p.n_gt = n_gt; p.n_thr = n_thr; p.img_h = img_h; p.img_w = img_w; p.single_cls = single_cls ? 1 : 0; p.eps = 1e-7f;
  p.tp = tp; p.conf = conf; p.cls = cls; p.status = status;
  if (mode == MODE_2D) hipLaunchKernelGGL(box_match_kernel<MODE_2D>, dim3(B), dim3(DM_BLOCK), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(box_match_kernel<MODE_3D>, dim3(B), dim3(DM_BLOCK), 0, (hipStream_t)stream, p);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_confusion_batch(int mode, const void* preds, const unsigned char* keep, int B, int K, const double* meta, int img_h, int img_w,
                        int single_cls, const float* gt_img, const float* gt_cls, const float* gt_box, int n_gt, int nc, double conf,
                        double iou_thres, int* matrix, int* status, void* stream) {
  Y3D_CHECK(mode == MODE_2D || mode == MODE_3D, "confusion_batch: mode must be 0 (2D) or 1 (3D), got %d", mode);
  Y3D_CHECK(K >= 0 && K <= DM_MAX_DET, "confusion_batch: %d detections per image (at most %d)", K, DM_MAX_DET);
  Y3D_CHECK(B >= 0 && n_gt >= 0 && nc >= 1 && (K == 0 || preds) && meta && matrix && status, "confusion_batch: bad arguments");
  Y3D_CHECK(n_gt == 0 || (gt_img && gt_cls && gt_box), "confusion_batch: null gt arrays");
  Y3D_CHECK(iou_thres >= 0.0, "confusion_batch: iou_thres must not be negative");
  if (B == 0) return Y3D_OK;
  ConfP p{};
  p.preds = preds; p.keep = keep; p.meta = meta; p.gt_img = gt_img; p.gt_cls = gt_cls; p.gt_box = gt_box;
  p.B = B; p.K = K; p.n_gt = n_gt; p.img_h = img_h; p.img_w = img_w; p.single_cls = single_cls ? 1 : 0; p.nc = nc;
  p.eps = 1e-7f; p.iou_thres = (float)iou_thres; p.conf = conf; p.matrix = matrix; p.status = status;
  if (mode == MODE_2D) hipLaunchKernelGGL(confusion_kernel<MODE_2D>, dim3(B), dim3(DM_BLOCK), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(confusion_kernel<MODE_3D>, dim3(B), dim3(DM_BLOCK), 0, (hipStream_t)stream, p);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_confusion_image(const float* gt_box, const int* gt_cls, int n_gt, const void* det, int det_f64, int n_det, int nc, double conf,
                        double iou_thres, int* matrix, int* status, void* stream) {
  Y3D_CHECK(n_gt >= 0 && n_gt <= DM_MAX_GT, "confusion_image: %d labels (at most %d)", n_gt, DM_MAX_GT);
  Y3D_CHECK(n_det >= 0 && n_det <= DM_MAX_DET, "confusion_image: %d detections (at most %d)", n_det, DM_MAX_DET);
  Y3D_CHECK(nc >= 1 && matrix && status && (n_gt == 0 || (gt_box && gt_cls)), "confusion_image: bad arguments");
  Y3D_CHECK(iou_thres >= 0.0, "confusion_image: iou_thres must not be negative");
  if (det == nullptr) n_det = 0;  // the validators' `detections=None`
  if (n_gt == 0 && n_det == 0) return Y3D_OK;
  ConfP p{};
  p.preds = det; p.gt_cls_i = gt_cls; p.gt_box = gt_box; p.det_f64 = det_f64 ? 1 : 0; p.count_empty = 1;
  p.B = 1; p.K = n_det; p.n_gt = n_gt; p.nc = nc;
  p.eps = 1e-7f; p.iou_thres = (float)iou_thres; p.conf = conf; p.matrix = matrix; p.status = status;
  hipLaunchKernelGGL(confusion_kernel<MODE_XYXY>, dim3(1), dim3(DM_BLOCK), 0, (hipStream_t)stream, p);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_ap_per_class(const int* tp, const double* conf, const int* cls, int64_t n, const int* ucls, const double* nl, int nc, int n_thr,
                     const double* x_ap, int n_ap, const double* x_curve, int n_curve, double* ap, double* p_curve, double* r_curve,
                     void* stream) {
  Y3D_CHECK(n >= 0 && (n == 0 || (tp && conf && cls)), "ap_per_class: bad detection arrays");
  Y3D_CHECK(nc >= 0 && n_thr >= 1 && n_thr <= DM_MAX_THR, "ap_per_class: %d classes, %d thresholds (1 .. %d)", nc, n_thr, DM_MAX_THR);
  Y3D_CHECK(n_ap >= 2 && n_ap <= DM_MAX_AP_PTS && n_curve >= 1 && n_curve <= DM_MAX_CURVE_PTS && x_ap && x_curve,
            "ap_per_class: grids of %d / %d points (2 .. %d / 1 .. %d)", n_ap, n_curve, DM_MAX_AP_PTS, DM_MAX_CURVE_PTS);
  if (nc == 0) return Y3D_OK;
  Y3D_CHECK(ucls && nl && ap && p_curve && r_curve, "ap_per_class: null output");
  ApP p{tp, conf, cls, (long)n, ucls, nl, n_thr, x_ap, n_ap, x_curve, n_curve, ap, p_curve, r_curve};
  hipLaunchKernelGGL(ap_kernel, dim3(nc, n_thr), dim3(DM_BLOCK), 0, (hipStream_t)stream, p);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

}  // extern "C"
