// KITTI 3D / BEV / 2D AP evaluation on the device (data/datasets/kitti_eval.py, the evaluator of KITTIDataset.get_stats):
//   * per-image (n_dt, n_gt) overlap blocks of the three metrics          (calculate_iou_partly :698-781, without the cross-image parts)
//   * compute_statistics_jit in both modes, ignore flags derived in-kernel (clean_data :369-425, compute_statistics_jit :518-636)
//   * fixed-order sum of the per-image counts over images                  (fused_compute_statistics :648-696)
// Everything is fp32 as the reference's float32 annos make it, with contraction off so the products that decide `overlap > min_overlap`
// round as the reference's; comparisons against the reference's float64 constants (min_overlap, the -1e-6 inclusion slack) are in double.
// No kernel uses scratch: every run-time indexed per-lane array (polygon, sort keys, assigned-detection bitmask) lives in an LDS slot.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int KE_MAX_BOX = 256;   // dets / gts per image
constexpr int KE_NPTS = 24;       // polygon candidates: 8 corners + 16 edge crossings
constexpr int KE_OV_BLOCK = 64;   // lanes of the overlap kernel (one polygon slot each)
constexpr int KE_ST_BLOCK = 256;  // max lanes of the statistics kernel (41 thresholds x <= 6 min-overlaps)
constexpr int KE_NT = 41;         // N_SAMPLE_PTS
constexpr int KE_BOX_F = 16;      // packed box record (see y3d.h)

// packed box record fields
enum { B_X1 = 0, B_Y1, B_X2, B_Y2, B_X, B_Y, B_Z, B_L, B_H, B_W, B_RY, B_ALPHA, B_SCORE, B_OCC, B_TRUNC };

// rbbox_to_corners (:150-172): (cx, cy, dx, dy, angle) -> 4 corners, clockwise, rotated clockwise
__device__ __forceinline__ void rbox_corners(float cx, float cy, float xd, float yd, float ang, float* px, float* py) {
  const float c = cosf(ang), s = sinf(ang);
  const float hx = -xd / 2.f, hy = -yd / 2.f;
  const float ax[4] = {hx, hx, -hx, -hx};
  const float ay[4] = {hy, -hy, -hy, hy};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    px[i] = c * ax[i] + s * ay[i] + cx;
    py[i] = -s * ax[i] + c * ay[i] + cy;
  }
}

// point_in_quadrilateral (:104-121); the -1e-6 slack is a float64 constant in the reference, so the test is in double
__device__ __forceinline__ bool in_quad(float x, float y, const float* qx, const float* qy) {
  const float ab0 = qx[1] - qx[0], ab1 = qy[1] - qy[0];
  const float ad0 = qx[3] - qx[0], ad1 = qy[3] - qy[0];
  const float ap0 = x - qx[0], ap1 = y - qy[0];
  const float abab = ab0 * ab0 + ab1 * ab1, abap = ab0 * ap0 + ab1 * ap1;
  const float adad = ad0 * ad0 + ad1 * ad1, adap = ad0 * ap0 + ad1 * ap1;
  const double eps = -1e-6;
  return (double)(abab - abap) >= eps && (double)abap >= eps && (double)(adad - adap) >= eps && (double)adap >= eps;
}

// line_segment_intersection (:61-101): edge i of quad 1 against edge j of quad 2
__device__ __forceinline__ bool seg_cross(const float* p1x, const float* p1y, const float* p2x, const float* p2y, int i, int j, float& ox,
                                          float& oy) {
  const float A0 = p1x[i], A1 = p1y[i], B0 = p1x[(i + 1) & 3], B1 = p1y[(i + 1) & 3];
  const float C0 = p2x[j], C1 = p2y[j], D0 = p2x[(j + 1) & 3], D1 = p2y[(j + 1) & 3];
  const float BA0 = B0 - A0, BA1 = B1 - A1, DA0 = D0 - A0, CA0 = C0 - A0, DA1 = D1 - A1, CA1 = C1 - A1;
  const bool acd = DA1 * CA0 > CA1 * DA0;
  const bool bcd = (D1 - B1) * (C0 - B0) > (C1 - B1) * (D0 - B0);
  if (acd == bcd) return false;
  const bool abc = CA1 * BA0 > BA1 * CA0;
  const bool abd = DA1 * BA0 > BA1 * DA0;
  if (abc == abd) return false;
  const float DC0 = D0 - C0, DC1 = D1 - C1;
  const float ABBA = A0 * B1 - B0 * A1, CDDC = C0 * D1 - D0 * C1;
  const float DH = BA1 * DC0 - BA0 * DC1;
  ox = (ABBA * DC0 - BA0 * CDDC) / DH;
  oy = (ABBA * DC1 - BA1 * CDDC) / DH;
  return true;
}

// A corner that coincides exactly with a corner of the other box is inside it.  The reference's absolute -1e-6 slack fails for a box's
// own far corner once the coordinates are tens of metres (fp32 rounding of abab - abap is ~1e-6 there), so identical boxes lost corners
// and scored far below 1; boxes whose corners differ are unaffected.
__device__ __forceinline__ bool is_corner(float x, float y, const float* qx, const float* qy) {
  bool hit = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) hit |= (x == qx[k]) & (y == qy[k]);
  return hit;
}

__device__ __forceinline__ float tri_area(float a0, float a1, float b0, float b1, float c0, float c1) {
  return ((a0 - c0) * (b1 - c1) - (a1 - c1) * (b0 - c0)) / 2.f;
}

// inter (:248-260): intersection area of two rotated rectangles.  The candidate points go to this lane's LDS slot (stride KE_OV_BLOCK),
// in the reference's order (quadrilateral_intersection :124-147), are sorted by the reference's insertion sort on the pseudo-angle
// (sort_vertex_in_convex_polygon :175-209) and fan-triangulated from the first point (area :219-225).
__device__ float rbox_inter(const float* r1, const float* r2, float* sx, float* sy, float* sk) {
  float ax[4], ay[4], bx[4], by[4];
  rbox_corners(r1[0], r1[1], r1[2], r1[3], r1[4], ax, ay);
  rbox_corners(r2[0], r2[1], r2[2], r2[3], r2[4], bx, by);
  int n = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (in_quad(ax[i], ay[i], bx, by) || is_corner(ax[i], ay[i], bx, by)) { sx[n * KE_OV_BLOCK] = ax[i]; sy[n * KE_OV_BLOCK] = ay[i]; ++n; }
    if (in_quad(bx[i], by[i], ax, ay) || is_corner(bx[i], by[i], ax, ay)) { sx[n * KE_OV_BLOCK] = bx[i]; sy[n * KE_OV_BLOCK] = by[i]; ++n; }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float ox, oy;
      if (seg_cross(ax, ay, bx, by, i, j, ox, oy)) { sx[n * KE_OV_BLOCK] = ox; sy[n * KE_OV_BLOCK] = oy; ++n; }
    }
  if (n <= 0) return 0.f;
  float cx = 0.f, cy = 0.f;
  for (int i = 0; i < n; ++i) { cx += sx[i * KE_OV_BLOCK]; cy += sy[i * KE_OV_BLOCK]; }
  cx /= (float)n;
  cy /= (float)n;
  for (int i = 0; i < n; ++i) {
    float vx = sx[i * KE_OV_BLOCK] - cx, vy = sy[i * KE_OV_BLOCK] - cy;
    const float d = sqrtf(vx * vx + vy * vy);
    vx = vx / d;
    vy = vy / d;
    if (vy < 0.f) vx = -2.f - vx;
    sk[i * KE_OV_BLOCK] = vx;
  }
  for (int i = 1; i < n; ++i) {
    const float t = sk[i * KE_OV_BLOCK];
    if (sk[(i - 1) * KE_OV_BLOCK] > t) {
      const float tx = sx[i * KE_OV_BLOCK], ty = sy[i * KE_OV_BLOCK];
      int j = i;
      while (j > 0 && sk[(j - 1) * KE_OV_BLOCK] > t) {
        sk[j * KE_OV_BLOCK] = sk[(j - 1) * KE_OV_BLOCK];
        sx[j * KE_OV_BLOCK] = sx[(j - 1) * KE_OV_BLOCK];
        sy[j * KE_OV_BLOCK] = sy[(j - 1) * KE_OV_BLOCK];
        --j;
      }
      sk[j * KE_OV_BLOCK] = t;
      sx[j * KE_OV_BLOCK] = tx;
      sy[j * KE_OV_BLOCK] = ty;
    }
  }
  float a = 0.f;
  const float x0 = sx[0], y0 = sy[0];
  for (int i = 0; i + 2 < n; ++i)
    a += fabsf(tri_area(x0, y0, sx[(i + 1) * KE_OV_BLOCK], sy[(i + 1) * KE_OV_BLOCK], sx[(i + 2) * KE_OV_BLOCK], sy[(i + 2) * KE_OV_BLOCK]));
  return a;
}

// one workgroup per image; lanes stride over the (dt, gt) pairs of its block
__global__ void __launch_bounds__(KE_OV_BLOCK) kitti_overlap_kernel(int metric, const float* __restrict__ gt, const float* __restrict__ dt,
                                                                    const int* __restrict__ gt_off, const int* __restrict__ dt_off,
                                                                    const int64_t* __restrict__ ov_off, float* __restrict__ out) {
  __shared__ float s_x[KE_NPTS * KE_OV_BLOCK], s_y[KE_NPTS * KE_OV_BLOCK], s_k[KE_NPTS * KE_OV_BLOCK];
  const int img = blockIdx.x, tid = threadIdx.x;
  const int g0 = gt_off[img], ng = gt_off[img + 1] - g0, d0 = dt_off[img], nd = dt_off[img + 1] - d0;
  float* o = out + ov_off[img];
  for (int p = tid; p < ng * nd; p += KE_OV_BLOCK) {
    const int j = p / ng, i = p - j * ng;  // dt j, gt i
    const float* G = gt + (size_t)(g0 + i) * KE_BOX_F;
    const float* D = dt + (size_t)(d0 + j) * KE_BOX_F;
    float ov = 0.f;
    if (metric == 0) {  // image_box_overlap(dt, gt) (:429-455), criterion -1
      const float qa = (G[B_X2] - G[B_X1]) * (G[B_Y2] - G[B_Y1]);
      const float iw = fminf(D[B_X2], G[B_X2]) - fmaxf(D[B_X1], G[B_X1]);
      if (iw > 0.f) {
        const float ih = fminf(D[B_Y2], G[B_Y2]) - fmaxf(D[B_Y1], G[B_Y1]);
        if (ih > 0.f) {
          const float ua = (D[B_X2] - D[B_X1]) * (D[B_Y2] - D[B_Y1]) + qa - iw * ih;
          ov = iw * ih / ua;
        }
      }
    } else {
      // BEV (x, z, l, w, ry); devRotateIoUEval(rbox1 = gt, rbox2 = dt) as rotate_iou_kernel_eval calls it with dt as `boxes`
      const float r1[5] = {G[B_X], G[B_Z], G[B_L], G[B_W], G[B_RY]};
      const float r2[5] = {D[B_X], D[B_Z], D[B_L], D[B_W], D[B_RY]};
      const float inter = rbox_inter(r1, r2, s_x + tid, s_y + tid, s_k + tid);
      if (metric == 1) {
        ov = inter / (r1[2] * r1[3] + r2[2] * r2[3] - inter);
      } else if (inter > 0.f) {  // box3d_overlap_kernel (:465-515), z_axis = 1, z_center = 1.0: y is the bottom face
        const float iw = fminf(D[B_Y], G[B_Y]) - fmaxf(D[B_Y] - D[B_H], G[B_Y] - G[B_H]);
        if (iw > 0.f) {
          const float a1 = D[B_L] * D[B_H] * D[B_W], a2 = G[B_L] * G[B_H] * G[B_W];
          const float inc = iw * inter;
          ov = inc / (a1 + a2 - inc);
        }
      }
    }
    o[p] = ov;
  }
}

// clean_data's tables (:369-425); class codes: 0 car 1 pedestrian 2 cyclist 3 van 4 person_sitting 5 tractor 6 trailer 7 other, +8 DontCare
__constant__ float kMinHeight[3] = {40.f, 25.f, 25.f};
__constant__ float kMaxOcc[3] = {0.f, 1.f, 2.f};
__constant__ double kMaxTrunc[3] = {0.15, 0.3, 0.5};

struct StatsP {
  const float* gt;
  const float* dt;
  const int* gt_code;
  const int* dt_code;
  const int* gt_off;
  const int* dt_off;
  const int64_t* ov_off;
  const float* ov;
  const int* cd;          // (ncd, 2) canonical class code, difficulty
  const double* min_ov;   // (ncd * nk)
  const float* thr;       // (ncd * nk, 41) counting pass
  const int* nthr;        // (ncd * nk)
  int n_img, nk, metric, compute_aos, total_gt;
  float* tp_score;        // (ncd * nk, total_gt) threshold pass: score of the det each gt is a true positive of
  int* nvalid;            // (ncd, n_img) threshold pass
  int* cnt;               // (ncd * nk, 41, n_img, 3) counting pass: tp, fp, fn
  double* sim;            // (ncd * nk, 41, n_img) counting pass: similarity, -1 when tp = fp = 0
};

// compute_statistics_jit (:518-636).  One workgroup per (image, class x difficulty); COUNT = false: lane k = min-overlap k, thresh 0;
// COUNT = true: lane = t * nk + k (41 thresholds x nk min-overlaps), so every lane walks the same gt / dt loops.
template <bool COUNT>
__global__ void __launch_bounds__(KE_ST_BLOCK) kitti_stats_kernel(StatsP p) {
  __shared__ signed char s_igt[KE_MAX_BOX], s_idt[KE_MAX_BOX];
  __shared__ float s_score[KE_MAX_BOX], s_dc[KE_MAX_BOX], s_galpha[KE_MAX_BOX], s_dalpha[KE_MAX_BOX];
  __shared__ unsigned s_asg[(KE_MAX_BOX / 32) * KE_ST_BLOCK];
  __shared__ int s_nvalid;
  const int img = blockIdx.x, cdi = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
  const int cls = p.cd[2 * cdi], diff = p.cd[2 * cdi + 1];
  const int g0 = p.gt_off[img], ng = p.gt_off[img + 1] - g0, d0 = p.dt_off[img], nd = p.dt_off[img + 1] - d0;
  if (ng > KE_MAX_BOX || nd > KE_MAX_BOX) return;  // refused by the host layer (y3d_kitti_eval_max_boxes); never index past the LDS tables
  if (tid == 0) s_nvalid = 0;
  __syncthreads();
  for (int i = tid; i < ng; i += nt) {
    const float* G = p.gt + (size_t)(g0 + i) * KE_BOX_F;
    const int code = p.gt_code[g0 + i] & 7;
    const int valid = code == cls ? 1 : ((cls == 1 && code == 4) || (cls == 0 && code == 3)) ? 0 : -1;
    const float h = G[B_Y2] - G[B_Y1];
    const bool ign = G[B_OCC] > kMaxOcc[diff] || (double)G[B_TRUNC] > kMaxTrunc[diff] || h <= kMinHeight[diff];
    const int f = (valid == 1 && !ign) ? 0 : (valid == 0 || (ign && valid == 1)) ? 1 : -1;
    s_igt[i] = (signed char)f;
    s_galpha[i] = G[B_ALPHA];
    if (!COUNT && f == 0) atomicAdd(&s_nvalid, 1);
  }
  for (int j = tid; j < nd; j += nt) {
    const float* D = p.dt + (size_t)(d0 + j) * KE_BOX_F;
    const float h = fabsf(D[B_Y2] - D[B_Y1]);
    s_idt[j] = (signed char)(h < kMinHeight[diff] ? 1 : (p.dt_code[d0 + j] & 7) == cls ? 0 : -1);
    s_score[j] = D[B_SCORE];
    s_dalpha[j] = D[B_ALPHA];
    // largest criterion-0 overlap with the image's DontCare boxes (image_box_overlap(dt, dc, 0) :604-617; dc boxes are float64 there)
    float dc = -INFINITY;
    if (COUNT && p.metric == 0) {
      const float ua = (D[B_X2] - D[B_X1]) * (D[B_Y2] - D[B_Y1]);
      for (int i = 0; i < ng; ++i) {
        if (!(p.gt_code[g0 + i] & 8)) continue;
        const float* C = p.gt + (size_t)(g0 + i) * KE_BOX_F;
        float o = 0.f;
        const double iw = fmin((double)D[B_X2], (double)C[B_X2]) - fmax((double)D[B_X1], (double)C[B_X1]);
        if (iw > 0.0) {
          const double ih = fmin((double)D[B_Y2], (double)C[B_Y2]) - fmax((double)D[B_Y1], (double)C[B_Y1]);
          if (ih > 0.0) o = (float)(iw * ih / (double)ua);
        }
        dc = fmaxf(dc, o);
      }
    }
    s_dc[j] = dc;
  }
  __syncthreads();
  if (!COUNT && tid == 0) p.nvalid[(size_t)cdi * p.n_img + img] = s_nvalid;
  const int lanes = COUNT ? KE_NT * p.nk : p.nk;
  if (tid >= lanes) return;
  const int k = tid % p.nk, t = COUNT ? tid / p.nk : 0;
  const int s = cdi * p.nk + k;
  if (COUNT && t >= p.nthr[s]) {
    const size_t o = ((size_t)s * KE_NT + t) * p.n_img + img;
    p.cnt[3 * o] = p.cnt[3 * o + 1] = p.cnt[3 * o + 2] = 0;
    p.sim[o] = 0.0;
    return;
  }
  const double mo = p.min_ov[s];
  const float thresh = COUNT ? p.thr[(size_t)s * KE_NT + t] : 0.f;
  const float* ov = p.ov + p.ov_off[img];
  unsigned* asg = s_asg + tid;
  for (int w = 0; w < (nd + 31) / 32; ++w) asg[w * KE_ST_BLOCK] = 0u;
  int tp = 0, fp = 0, fn = 0;
  double simsum = 0.0;
  for (int i = 0; i < ng; ++i) {
    const int ig = s_igt[i];
    if (ig == -1) continue;
    int det = -1;
    bool valid = false, aid = false;
    float vscore = -10000000.f, maxov = 0.f;
    for (int j = 0; j < nd; ++j) {
      const int id = s_idt[j];
      if (id == -1) continue;
      if ((asg[(j >> 5) * KE_ST_BLOCK] >> (j & 31)) & 1u) continue;
      const float sc = s_score[j];
      if (COUNT && sc < thresh) continue;
      const float o = ov[(size_t)j * ng + i];
      const bool above = (double)o > mo;
      if (!COUNT) {
        if (above && sc > vscore) { det = j; vscore = sc; valid = true; }
      } else if (above && (o > maxov || aid) && id == 0) {
        maxov = o; det = j; valid = true; aid = false;
      } else if (above && !valid && id == 1) {
        det = j; valid = true; aid = true;
      }
    }
    if (!valid) {
      if (ig == 0) ++fn;
    } else {
      if (!(ig == 1 || s_idt[det] == 1)) {
        ++tp;
        if (!COUNT) p.tp_score[(size_t)s * p.total_gt + g0 + i] = s_score[det];
        if (COUNT && p.compute_aos) simsum += (1.0 + cos((double)(s_galpha[i] - s_dalpha[det]))) / 2.0;
      }
      asg[(det >> 5) * KE_ST_BLOCK] |= 1u << (det & 31);
    }
  }
  if (!COUNT) return;
  for (int j = 0; j < nd; ++j) {
    if (s_idt[j] != 0 || ((asg[(j >> 5) * KE_ST_BLOCK] >> (j & 31)) & 1u) || s_score[j] < thresh) continue;
    if (p.metric == 0 && (double)s_dc[j] > mo) continue;  // DontCare suppression: counted, then subtracted as `nstuff`
    ++fp;
  }
  const size_t o = ((size_t)s * KE_NT + t) * p.n_img + img;
  p.cnt[3 * o] = tp;
  p.cnt[3 * o + 1] = fp;
  p.cnt[3 * o + 2] = fn;
  p.sim[o] = !p.compute_aos ? 0.0 : (tp > 0 || fp > 0) ? simsum : -1.0;
}

// pr[s, t] = sum over images (fused_compute_statistics :681-684): one workgroup per (s, t), strided partial sums then a fixed tree
__global__ void __launch_bounds__(256) kitti_pr_reduce_kernel(const int* __restrict__ cnt, const double* __restrict__ sim, int n_img,
                                                              double* __restrict__ pr) {
  __shared__ long long s_c[3][256];
  __shared__ double s_s[256];
  const int st = blockIdx.x, tid = threadIdx.x;
  long long c0 = 0, c1 = 0, c2 = 0;
  double sv = 0.0;
  for (int i = tid; i < n_img; i += 256) {
    const size_t o = (size_t)st * n_img + i;
    c0 += cnt[3 * o];
    c1 += cnt[3 * o + 1];
    c2 += cnt[3 * o + 2];
    const double v = sim[o];
    if (v != -1.0) sv += v;
  }
  s_c[0][tid] = c0; s_c[1][tid] = c1; s_c[2][tid] = c2; s_s[tid] = sv;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) {
      s_c[0][tid] += s_c[0][tid + h];
      s_c[1][tid] += s_c[1][tid + h];
      s_c[2][tid] += s_c[2][tid + h];
      s_s[tid] += s_s[tid + h];
    }
    __syncthreads();
  }
  if (tid == 0) {
    pr[4 * (size_t)st] = (double)s_c[0][0];
    pr[4 * (size_t)st + 1] = (double)s_c[1][0];
    pr[4 * (size_t)st + 2] = (double)s_c[2][0];
    pr[4 * (size_t)st + 3] = s_s[0];
  }
}

}  // namespace

extern "C" {

int y3d_kitti_eval_max_boxes(void) { return KE_MAX_BOX; }

int y3d_kitti_box_overlaps(int metric, const float* gt, const float* dt, const int* gt_off, const int* dt_off, const int64_t* ov_off,
                           int n_img, float* out, void* stream) {
  Y3D_CHECK(metric >= 0 && metric <= 2, "kitti_box_overlaps: metric must be 0 (2D), 1 (BEV) or 2 (3D), got %d", metric);
  Y3D_CHECK(n_img >= 1 && gt_off && dt_off && ov_off && out, "kitti_box_overlaps: bad arguments");
  hipLaunchKernelGGL(kitti_overlap_kernel, dim3(n_img), dim3(KE_OV_BLOCK), 0, (hipStream_t)stream, metric, gt, dt, gt_off, dt_off, ov_off, out);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

static int kitti_stats_args(const char* who, int metric, int n_img, int ncd, int nk, const int* cd) {
  Y3D_CHECK(metric >= 0 && metric <= 2, "%s: bad metric %d", who, metric);
  Y3D_CHECK(n_img >= 1 && ncd >= 1 && cd, "%s: bad sizes", who);
  Y3D_CHECK(nk >= 1 && KE_NT * nk <= KE_ST_BLOCK, "%s: %d min-overlaps (1 .. %d supported)", who, nk, KE_ST_BLOCK / KE_NT);
  return Y3D_OK;
}

int y3d_kitti_eval_thresholds(const float* gt, const int* gt_code, const float* dt, const int* dt_code, const int* gt_off, const int* dt_off,
                              const int64_t* ov_off, const float* ov, int n_img, int total_gt, int metric, const int* cd, int ncd,
                              const double* min_ov, int nk, float* tp_score, int* nvalid, void* stream) {
  if (kitti_stats_args("kitti_eval_thresholds", metric, n_img, ncd, nk, cd)) return Y3D_ERR_INVALID;
  Y3D_CHECK(tp_score && nvalid && min_ov, "kitti_eval_thresholds: null output");
  StatsP p{gt, dt, gt_code, dt_code, gt_off, dt_off, ov_off, ov, cd, min_ov, nullptr, nullptr, n_img, nk, metric, 0, total_gt,
           tp_score, nvalid, nullptr, nullptr};
  hipLaunchKernelGGL(kitti_stats_kernel<false>, dim3(n_img, ncd), dim3(64), 0, (hipStream_t)stream, p);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_kitti_eval_counts(const float* gt, const int* gt_code, const float* dt, const int* dt_code, const int* gt_off, const int* dt_off,
                          const int64_t* ov_off, const float* ov, int n_img, int metric, const int* cd, int ncd, const double* min_ov, int nk,
                          const float* thr, const int* nthr, int compute_aos, int* cnt, double* sim, double* pr, void* stream) {
  if (kitti_stats_args("kitti_eval_counts", metric, n_img, ncd, nk, cd)) return Y3D_ERR_INVALID;
  Y3D_CHECK(thr && nthr && cnt && sim && pr && min_ov, "kitti_eval_counts: null argument");
  StatsP p{gt, dt, gt_code, dt_code, gt_off, dt_off, ov_off, ov, cd, min_ov, thr, nthr, n_img, nk, metric, compute_aos ? 1 : 0, 0,
           nullptr, nullptr, cnt, sim};
  const int lanes = (KE_NT * nk + 63) / 64 * 64;
  hipLaunchKernelGGL(kitti_stats_kernel<true>, dim3(n_img, ncd), dim3(lanes), 0, (hipStream_t)stream, p);
  Y3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(kitti_pr_reduce_kernel, dim3(ncd * nk * KE_NT), dim3(256), 0, (hipStream_t)stream, cnt, sim, n_img, pr);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

}  // extern "C"
