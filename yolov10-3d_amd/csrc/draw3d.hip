// Drawing 3D predictions on the device (plot.py): box wireframes over the camera image and filled boxes on a bird's-eye-view map.
// Two prepare kernels turn `y3d_predict3d_rows`' outputs into primitive tables, two raster kernels paint such tables into a uint8 NHWC
// canvas.  Everything is float64 with FMA contraction off and every sum is evaluated left to right as written below, so a few lines of
// NumPy (tests/draw_ref.py) give the same bytes.  Pixel (x, y) is the point (x, y): integer coordinates are pixel centres.
//
// y3d_box3d_segments — one thread per box.  The eight corners (generate_corners3d's order) go to homogeneous image coordinates with the
//   full 3 x 4 P2, U = ((P0 x + P1 y) + P2 z) + P3 (V, W from rows 1, 2).  The 14 segments are the bottom face 0-1 1-2 2-3 3-0, the top
//   face 4-5 5-6 6-7 7-4, the uprights 0-4 1-5 2-6 3-7 and the front face's diagonals 0-5 1-4 (they mark the heading).  A segment with
//   both W < near is dropped; with one W < near that endpoint A becomes A + s (B - A) in (U, V, W), s = (near - W_A) / (W_B - W_A);
//   W == near is kept.  Then u = U / W, v = V / W, then the optional affine u' = (A00 u + A01 v) + A02, v' = (A10 u + A11 v) + A12.
//   Dropped segments and the slots of boxes behind counts[b] are NaN (slot k * 14 + j always belongs to box k).  The colour of a box is
//   palette[clamp((int)cls, 0, n_pal - 1)], a NaN class taking entry 0 (every box with rows NULL); the fourth colour byte is 0.
// y3d_box3d_bev_quads — one thread per box: the bottom face's corners 0..3 as (cx + scale x, cy - scale z).
//
// y3d_draw_segments / y3d_draw_quads — a gather: one workgroup of 256 threads per 64 x 16 pixel tile of its image (a wave is one
//   64-pixel row, a thread owns four rows), grid (tiles x, tiles y, B).  The image's primitives are walked in chunks of 256: each thread
//   tests one primitive's bounding box, widened by thickness / 2 + 1 pixel, against the tile (a primitive with a non-finite coordinate,
//   or a quad of area 0, never passes); the survivors are compacted IN INDEX ORDER into an LDS list (ballot + popcount, the scheme of
//   predict3d_rows_kernel) with what depends on the primitive alone (d, len2, r2 len2; the quad's edges) computed once; every pixel
//   thread walks the list from its start and stops at its first hit, so the primitive with the lowest index wins a pixel, chunk after
//   chunk (a done bit per pixel survives the chunks).  Only covered pixels are stored.  No atomics, no second buffer: the canvas after
//   the call is a function of the inputs alone.
//
//   segment a -> b, thickness t, r2 = (t/2)(t/2), pixel p:  d = b - a, e = p - a, len2 = d.x d.x + d.y d.y, dot = e.x d.x + e.y d.y;
//     dot <= 0: covered iff e.x e.x + e.y e.y <= r2;  dot >= len2: the same with p - b;  else c = d.x e.y - d.y e.x, covered iff
//     c c <= r2 len2.  No division, no square root; len2 == 0 is a disc.
//   quad q0..q3, pixel p:  E_i = (q_{i+1} - q_i) x (p - q_i) = d_i.x (p.y - q_i.y) - d_i.y (p.x - q_i.x); covered iff all four E_i >= 0
//     or all four <= 0 (both windings).  Skipped when (q1 - q0) x (q2 - q0) + (q2 - q0) x (q3 - q0), its doubled signed area, is 0.
//
// The bounding-box cull is exact for coordinates up to 1e12 in magnitude (the rounding of the coverage sums then stays far below the
// extra pixel of the margin); beyond that the squares of the rule itself lose their meaning long before they overflow.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TW = 64, TH = 16, CH = 256;  // tile width / height in pixels, primitives per chunk (= threads)

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }  // false for NaN and +-inf

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

__device__ __forceinline__ unsigned box_colour(double cls, const unsigned char* __restrict__ palette, int n_pal) {
  int i = 0;  // NaN fails both comparisons
  if (cls >= (double)(n_pal - 1)) i = n_pal - 1;
  else if (cls > 0.0) i = (int)cls;
  const unsigned char* p = palette + (size_t)i * 3;
  return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
}

struct Affine {
  double a00, a01, a02, a10, a11, a12;
  bool on;
};

__device__ __forceinline__ void emit_segment(double2* __restrict__ os, int j, double Ua, double Va, double Wa, double Ub, double Vb,
                                             double Wb, double nearw, const Affine& A) {
  const bool la = Wa < nearw, lb = Wb < nearw;
  double ax = quiet_nan(), ay = ax, bx = ax, by = ax;
  if (!(la && lb)) {
    if (la) {
      const double s = (nearw - Wa) / (Wb - Wa);
      Ua = Ua + s * (Ub - Ua);
      Va = Va + s * (Vb - Va);
      Wa = Wa + s * (Wb - Wa);
    } else if (lb) {
      const double s = (nearw - Wb) / (Wa - Wb);
      Ub = Ub + s * (Ua - Ub);
      Vb = Vb + s * (Va - Vb);
      Wb = Wb + s * (Wa - Wb);
    }
    ax = Ua / Wa;
    ay = Va / Wa;
    bx = Ub / Wb;
    by = Vb / Wb;
    if (A.on) {
      const double u0 = (A.a00 * ax + A.a01 * ay) + A.a02, v0 = (A.a10 * ax + A.a11 * ay) + A.a12;
      const double u1 = (A.a00 * bx + A.a01 * by) + A.a02, v1 = (A.a10 * bx + A.a11 * by) + A.a12;
      ax = u0, ay = v0, bx = u1, by = v1;
    }
  }
  os[2 * j] = make_double2(ax, ay);
  os[2 * j + 1] = make_double2(bx, by);
}

__global__ void __launch_bounds__(256) box3d_segments_kernel(const double* __restrict__ corners3d, const double* __restrict__ rows,
                                                           const int* __restrict__ counts, int B, int K, const double* __restrict__ P2,
                                                           const double* __restrict__ affine, const unsigned char* __restrict__ palette,
                                                           int n_pal, double nearw, double* __restrict__ segs, unsigned* __restrict__ seg_rgb) {
  const int i = blockIdx.x * 256 + threadIdx.x;  // B * K * 14 fits an int (checked by the entry)
  if (i >= B * K) return;
  const int b = i / K, k = i - b * K;
  double2* os = (double2*)(segs + (size_t)i * 56);
  unsigned* oc = seg_rgb + (size_t)i * 14;
  if (k >= counts[b]) {
    const double2 n2 = make_double2(quiet_nan(), quiet_nan());
#pragma unroll
    for (int j = 0; j < 28; ++j) os[j] = n2;
#pragma unroll
    for (int j = 0; j < 14; ++j) oc[j] = 0u;
    return;
  }
  const double* P = P2 + (size_t)b * 12;
  const double p00 = P[0], p01 = P[1], p02 = P[2], p03 = P[3], p10 = P[4], p11 = P[5], p12 = P[6], p13 = P[7], p20 = P[8], p21 = P[9],
               p22 = P[10], p23 = P[11];
  Affine A = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, affine != nullptr};
  if (affine) {
    const double* a = affine + (size_t)b * 6;
    A.a00 = a[0], A.a01 = a[1], A.a02 = a[2], A.a10 = a[3], A.a11 = a[4], A.a12 = a[5];
  }
  const double2* c3 = (const double2*)(corners3d + (size_t)i * 24);
  double v[24], U[8], V[8], Wc[8];
#pragma unroll
  for (int q = 0; q < 12; ++q) {
    const double2 t = c3[q];
    v[2 * q] = t.x, v[2 * q + 1] = t.y;
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const double x = v[c * 3], y = v[c * 3 + 1], z = v[c * 3 + 2];
    U[c] = ((p00 * x + p01 * y) + p02 * z) + p03;
    V[c] = ((p10 * x + p11 * y) + p12 * z) + p13;
    Wc[c] = ((p20 * x + p21 * y) + p22 * z) + p23;
  }
  const unsigned rgb = box_colour(rows ? rows[(size_t)i * 14] : 0.0, palette, n_pal);
#define Y3D_SEG(j, a, c) emit_segment(os, j, U[a], V[a], Wc[a], U[c], V[c], Wc[c], nearw, A)
  Y3D_SEG(0, 0, 1); Y3D_SEG(1, 1, 2); Y3D_SEG(2, 2, 3); Y3D_SEG(3, 3, 0);
  Y3D_SEG(4, 4, 5); Y3D_SEG(5, 5, 6); Y3D_SEG(6, 6, 7); Y3D_SEG(7, 7, 4);
  Y3D_SEG(8, 0, 4); Y3D_SEG(9, 1, 5); Y3D_SEG(10, 2, 6); Y3D_SEG(11, 3, 7);
  Y3D_SEG(12, 0, 5); Y3D_SEG(13, 1, 4);
#undef Y3D_SEG
#pragma unroll
  for (int j = 0; j < 14; ++j) oc[j] = rgb;
}

__global__ void __launch_bounds__(256) box3d_bev_quads_kernel(const double* __restrict__ corners3d, const double* __restrict__ rows,
                                                            const int* __restrict__ counts, int B, int K,
                                                            const unsigned char* __restrict__ palette, int n_pal, double scale, double cx,
                                                            double cy, double* __restrict__ quads, unsigned* __restrict__ quad_rgb) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * K) return;
  const int b = i / K, k = i - b * K;
  double2* oq = (double2*)(quads + (size_t)i * 8);
  if (k >= counts[b]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) oq[c] = make_double2(quiet_nan(), quiet_nan());
    quad_rgb[i] = 0u;
    return;
  }
  const double* c3 = corners3d + (size_t)i * 24;
#pragma unroll
  for (int c = 0; c < 4; ++c) oq[c] = make_double2(cx + scale * c3[c * 3], cy - scale * c3[c * 3 + 2]);
  quad_rgb[i] = box_colour(rows ? rows[(size_t)i * 14] : 0.0, palette, n_pal);
}

// this thread's slot among the chunk's survivors, in thread (= index) order, or -1; total = survivors of the chunk (block-uniform)
__device__ __forceinline__ int compact_slot(bool keep, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wsum[wave] = __popcll(m);
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    before += w < wave ? wsum[w] : 0;
    all += wsum[w];
  }
  total = all;
  return keep ? before + __popcll(m & ((1ull << lane) - 1ull)) : -1;
}

struct Tile {
  int px, py0, done;  // this thread's column, its first row (rows py0 + 4 i), bit i set = pixel i needs no more tests
  double x0, x1, y0, y1;  // the tile's first and last pixel centres
};

__device__ __forceinline__ Tile make_tile(int H, int W) {
  Tile t;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  t.px = x0 + (threadIdx.x & 63);
  t.py0 = y0 + (threadIdx.x >> 6);
  t.done = t.px < W ? 0 : 15;
#pragma unroll
  for (int i = 0; i < 4; ++i) t.done |= (t.py0 + 4 * i < H) ? 0 : (1 << i);
  t.x0 = (double)x0, t.x1 = (double)min(x0 + TW - 1, W - 1);
  t.y0 = (double)y0, t.y1 = (double)min(y0 + TH - 1, H - 1);
  return t;
}

__device__ __forceinline__ void put_pixel(unsigned char* __restrict__ img, int W, int x, int y, unsigned c) {
  unsigned char* o = img + ((size_t)y * W + x) * 3;  // x < W, y < H: the done bits of make_tile
  o[0] = (unsigned char)(c & 255u), o[1] = (unsigned char)((c >> 8) & 255u), o[2] = (unsigned char)((c >> 16) & 255u);
}

__global__ void __launch_bounds__(256) draw_segments_kernel(unsigned char* __restrict__ canvas, int H, int W, const double* __restrict__ segs,
                                                          const unsigned* __restrict__ seg_rgb, const int* __restrict__ nseg, int S,
                                                          double r2, double margin) {
  __shared__ double ls[CH][8];  // ax, ay, bx, by, dx, dy, len2, r2 * len2
  __shared__ unsigned lc[CH];
  __shared__ int wsum[4];
  const int b = blockIdx.z, t = threadIdx.x;
  const int n = nseg ? min(max(nseg[b], 0), S) : S;
  Tile T = make_tile(H, W);
  const double fx = (double)T.px;
  unsigned char* img = canvas + (size_t)b * H * W * 3;
  const double2* in = (const double2*)(segs + (size_t)b * S * 4);
  const unsigned* inc = seg_rgb + (size_t)b * S;
  for (int c0 = 0; c0 < n; c0 += CH) {
    const int s = c0 + t;
    bool keep = false;
    double ax = 0, ay = 0, bx = 0, by = 0;
    if (s < n) {
      const double2 a = in[2 * (size_t)s], e = in[2 * (size_t)s + 1];
      ax = a.x, ay = a.y, bx = e.x, by = e.y;
      keep = finite_d(ax) && finite_d(ay) && finite_d(bx) && finite_d(by) && fmin(ax, bx) - margin <= T.x1 && fmax(ax, bx) + margin >= T.x0 &&
             fmin(ay, by) - margin <= T.y1 && fmax(ay, by) + margin >= T.y0;
    }
    int cnt;
    const int slot = compact_slot(keep, wsum, cnt);
    if (slot >= 0) {  // slot < CH
      const double dx = bx - ax, dy = by - ay;
      const double len2 = dx * dx + dy * dy;
      ls[slot][0] = ax, ls[slot][1] = ay, ls[slot][2] = bx, ls[slot][3] = by;
      ls[slot][4] = dx, ls[slot][5] = dy, ls[slot][6] = len2, ls[slot][7] = r2 * len2;
      lc[slot] = inc[s];
    }
    __syncthreads();
    if (cnt > 0 && T.done != 15) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (T.done & (1 << i)) continue;
        const int y = T.py0 + 4 * i;
        const double fy = (double)y;
        for (int j = 0; j < cnt; ++j) {
          const double dx = ls[j][4], dy = ls[j][5], len2 = ls[j][6];
          const double ex = fx - ls[j][0], ey = fy - ls[j][1];
          const double dot = ex * dx + ey * dy;
          bool cov;
          if (dot <= 0.0) {
            cov = ex * ex + ey * ey <= r2;
          } else if (dot >= len2) {
            const double gx = fx - ls[j][2], gy = fy - ls[j][3];
            cov = gx * gx + gy * gy <= r2;
          } else {
            const double c = dx * ey - dy * ex;
            cov = c * c <= ls[j][7];
          }
          if (cov) {
            put_pixel(img, W, T.px, y, lc[j]);
            T.done |= 1 << i;
            break;
          }
        }
      }
    }
    __syncthreads();  // the list and wsum are rewritten by the next chunk
  }
}

__global__ void __launch_bounds__(256) draw_quads_kernel(unsigned char* __restrict__ canvas, int H, int W, const double* __restrict__ quads,
                                                       const unsigned* __restrict__ quad_rgb, const int* __restrict__ nquad, int Q) {
  __shared__ double lq[CH][16];  // q0..q3 (x, y), then the edges d_i = q_{i+1} - q_i (x, y)
  __shared__ unsigned lc[CH];
  __shared__ int wsum[4];
  const int b = blockIdx.z, t = threadIdx.x;
  const int n = nquad ? min(max(nquad[b], 0), Q) : Q;
  Tile T = make_tile(H, W);
  const double fx = (double)T.px;
  unsigned char* img = canvas + (size_t)b * H * W * 3;
  const double2* in = (const double2*)(quads + (size_t)b * Q * 8);
  const unsigned* inc = quad_rgb + (size_t)b * Q;
  for (int c0 = 0; c0 < n; c0 += CH) {
    const int s = c0 + t;
    bool keep = false;
    double2 q0 = make_double2(0, 0), q1 = q0, q2 = q0, q3 = q0;
    if (s < n) {
      q0 = in[4 * (size_t)s], q1 = in[4 * (size_t)s + 1], q2 = in[4 * (size_t)s + 2], q3 = in[4 * (size_t)s + 3];
      const bool fin = finite_d(q0.x) && finite_d(q0.y) && finite_d(q1.x) && finite_d(q1.y) && finite_d(q2.x) && finite_d(q2.y) &&
                       finite_d(q3.x) && finite_d(q3.y);
      const double ux = q1.x - q0.x, uy = q1.y - q0.y, vx = q2.x - q0.x, vy = q2.y - q0.y, wx = q3.x - q0.x, wy = q3.y - q0.y;
      const double area2 = (ux * vy - uy * vx) + (vx * wy - vy * wx);
      keep = fin && area2 != 0.0 && fmin(fmin(q0.x, q1.x), fmin(q2.x, q3.x)) - 1.0 <= T.x1 &&
             fmax(fmax(q0.x, q1.x), fmax(q2.x, q3.x)) + 1.0 >= T.x0 && fmin(fmin(q0.y, q1.y), fmin(q2.y, q3.y)) - 1.0 <= T.y1 &&
             fmax(fmax(q0.y, q1.y), fmax(q2.y, q3.y)) + 1.0 >= T.y0;
    }
    int cnt;
    const int slot = compact_slot(keep, wsum, cnt);
    if (slot >= 0) {
      double* l = lq[slot];
      l[0] = q0.x, l[1] = q0.y, l[2] = q1.x, l[3] = q1.y, l[4] = q2.x, l[5] = q2.y, l[6] = q3.x, l[7] = q3.y;
      l[8] = q1.x - q0.x, l[9] = q1.y - q0.y, l[10] = q2.x - q1.x, l[11] = q2.y - q1.y;
      l[12] = q3.x - q2.x, l[13] = q3.y - q2.y, l[14] = q0.x - q3.x, l[15] = q0.y - q3.y;
      lc[slot] = inc[s];
    }
    __syncthreads();
    if (cnt > 0 && T.done != 15) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (T.done & (1 << i)) continue;
        const int y = T.py0 + 4 * i;
        const double fy = (double)y;
        for (int j = 0; j < cnt; ++j) {
          const double* l = lq[j];
          const double e0 = l[8] * (fy - l[1]) - l[9] * (fx - l[0]);
          const double e1 = l[10] * (fy - l[3]) - l[11] * (fx - l[2]);
          const double e2 = l[12] * (fy - l[5]) - l[13] * (fx - l[4]);
          const double e3 = l[14] * (fy - l[7]) - l[15] * (fx - l[6]);
          if ((e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0 && e3 >= 0.0) || (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0 && e3 <= 0.0)) {
            put_pixel(img, W, T.px, y, lc[j]);
            T.done |= 1 << i;
            break;
          }
        }
      }
    }
    __syncthreads();
  }
}

struct Span {
  const void* p;
  size_t bytes;
};

// byte ranges, as y3d_predict3d_rows compares them; a NULL or empty range overlaps nothing
inline bool overlaps(const Span& a, const Span& b) {
  const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
  return a.p && b.p && a.bytes && b.bytes && a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

inline bool finite_h(double x) { return x - x == 0.0; }

}  // namespace

extern "C" {

int y3d_box3d_segments(const double* corners3d, const double* rows, const int* counts, int B, int K, const double* P2, const double* affine,
                       const unsigned char* palette, int n_pal, double near_w, double* segs, unsigned char* seg_rgb, void* stream) {
  Y3D_CHECK(B >= 1 && K >= 0 && n_pal >= 1, "box3d_segments: bad sizes (B >= 1, K >= 0, n_pal >= 1)");
  Y3D_CHECK((long)B * K * 14 <= 0x7fffffffL, "box3d_segments: B * K * 14 must fit an int");
  Y3D_CHECK(near_w == near_w, "box3d_segments: near is NaN");
  if (K == 0) return Y3D_OK;
  Y3D_CHECK(corners3d && counts && P2 && palette && segs && seg_rgb, "box3d_segments: null argument");
  Y3D_CHECK((((uintptr_t)corners3d | (uintptr_t)segs) & 15) == 0 && ((uintptr_t)seg_rgb & 3) == 0,
            "box3d_segments: corners3d and segs must be 16-byte aligned, seg_rgb 4-byte aligned");
  const size_t rk = (size_t)B * K;
  const Span ins[] = {{corners3d, rk * 192}, {rows, rk * 112}, {counts, (size_t)B * 4}, {P2, (size_t)B * 96},
                      {affine, (size_t)B * 48}, {palette, (size_t)n_pal * 3}};
  const Span outs[] = {{segs, rk * 14 * 32}, {seg_rgb, rk * 14 * 4}};
  for (const Span& o : outs)
    for (const Span& i : ins) Y3D_CHECK(!overlaps(o, i), "box3d_segments: an output overlaps an input");
  Y3D_CHECK(!overlaps(outs[0], outs[1]), "box3d_segments: the outputs overlap each other");
  hipLaunchKernelGGL(box3d_segments_kernel, dim3(cdiv((long)rk, 256)), dim3(256), 0, (hipStream_t)stream, corners3d, rows, counts, B, K, P2,
                     affine, palette, n_pal, near_w, segs, (unsigned*)seg_rgb);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_box3d_bev_quads(const double* corners3d, const double* rows, const int* counts, int B, int K, const unsigned char* palette,
                        int n_pal, double scale, double cx, double cy, double* quads, unsigned char* quad_rgb, void* stream) {
  Y3D_CHECK(B >= 1 && K >= 0 && n_pal >= 1, "box3d_bev_quads: bad sizes (B >= 1, K >= 0, n_pal >= 1)");
  Y3D_CHECK((long)B * K <= 0x7fffffffL, "box3d_bev_quads: B * K must fit an int");
  if (K == 0) return Y3D_OK;
  Y3D_CHECK(corners3d && counts && palette && quads && quad_rgb, "box3d_bev_quads: null argument");
  Y3D_CHECK(((uintptr_t)quads & 15) == 0 && ((uintptr_t)quad_rgb & 3) == 0,
            "box3d_bev_quads: quads must be 16-byte aligned, quad_rgb 4-byte aligned");
  const size_t rk = (size_t)B * K;
  const Span ins[] = {{corners3d, rk * 192}, {rows, rk * 112}, {counts, (size_t)B * 4}, {palette, (size_t)n_pal * 3}};
  const Span outs[] = {{quads, rk * 64}, {quad_rgb, rk * 4}};
  for (const Span& o : outs)
    for (const Span& i : ins) Y3D_CHECK(!overlaps(o, i), "box3d_bev_quads: an output overlaps an input");
  Y3D_CHECK(!overlaps(outs[0], outs[1]), "box3d_bev_quads: the outputs overlap each other");
  hipLaunchKernelGGL(box3d_bev_quads_kernel, dim3(cdiv((long)rk, 256)), dim3(256), 0, (hipStream_t)stream, corners3d, rows, counts, B, K,
                     palette, n_pal, scale, cx, cy, quads, (unsigned*)quad_rgb);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_draw_segments(unsigned char* canvas, int B, int H, int W, const double* segs, const unsigned char* seg_rgb, const int* nseg, int S,
                      double thickness, void* stream) {
  Y3D_CHECK(B >= 1 && H >= 1 && W >= 1 && S >= 0, "draw_segments: bad sizes (B, H, W >= 1, S >= 0)");
  Y3D_CHECK(finite_h(thickness) && thickness > 0.0, "draw_segments: the thickness must be finite and > 0");
  Y3D_CHECK(B <= 65535 && cdiv(H, TH) <= 65535, "draw_segments: at most 65535 images of at most %d rows", 65535 * TH);
  Y3D_CHECK(canvas, "draw_segments: null canvas");
  if (S == 0) return Y3D_OK;
  Y3D_CHECK(segs && seg_rgb, "draw_segments: null argument");
  Y3D_CHECK(((uintptr_t)segs & 15) == 0 && ((uintptr_t)seg_rgb & 3) == 0, "draw_segments: segs must be 16-byte aligned, seg_rgb 4-byte aligned");
  const Span cv = {canvas, (size_t)B * H * W * 3};
  const Span ins[] = {{segs, (size_t)B * S * 32}, {seg_rgb, (size_t)B * S * 4}, {nseg, (size_t)B * 4}};
  for (const Span& i : ins) Y3D_CHECK(!overlaps(cv, i), "draw_segments: the canvas overlaps an input");
  const double h = thickness / 2;
  hipLaunchKernelGGL(draw_segments_kernel, dim3(cdiv(W, TW), cdiv(H, TH), B), dim3(256), 0, (hipStream_t)stream, canvas, H, W, segs,
                     (const unsigned*)seg_rgb, nseg, S, h * h, h + 1.0);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_draw_quads(unsigned char* canvas, int B, int H, int W, const double* quads, const unsigned char* quad_rgb, const int* nquad, int Q,
                   void* stream) {
  Y3D_CHECK(B >= 1 && H >= 1 && W >= 1 && Q >= 0, "draw_quads: bad sizes (B, H, W >= 1, Q >= 0)");
  Y3D_CHECK(B <= 65535 && cdiv(H, TH) <= 65535, "draw_quads: at most 65535 images of at most %d rows", 65535 * TH);
  Y3D_CHECK(canvas, "draw_quads: null canvas");
  if (Q == 0) return Y3D_OK;
  Y3D_CHECK(quads && quad_rgb, "draw_quads: null argument");
  Y3D_CHECK(((uintptr_t)quads & 15) == 0 && ((uintptr_t)quad_rgb & 3) == 0, "draw_quads: quads must be 16-byte aligned, quad_rgb 4-byte aligned");
  const Span cv = {canvas, (size_t)B * H * W * 3};
  const Span ins[] = {{quads, (size_t)B * Q * 64}, {quad_rgb, (size_t)B * Q * 4}, {nquad, (size_t)B * 4}};
  for (const Span& i : ins) Y3D_CHECK(!overlaps(cv, i), "draw_quads: the canvas overlaps an input");
  hipLaunchKernelGGL(draw_quads_kernel, dim3(cdiv(W, TW), cdiv(H, TH), B), dim3(256), 0, (hipStream_t)stream, canvas, H, W, quads,
                     (const unsigned*)quad_rgb, nquad, Q);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

}  // extern "C"
