// GroupNorm over the raw output of a biased convolution, forward and backward, for the 3D head's depth predictor
// (nn/modules/head.py:978-1042 DepthPredictor: Conv2d + GroupNorm(32, 128) pairs; modules.DepthPredictor, ops.GroupNormFn).
//
// The convolution writes y WITHOUT its bias (the raw epilogue keeps the fast 3x3 / streaming 1x1 routes); these kernels add it:
//   x = y + b_conv[c],  xhat = (x - mean[b, g]) * rstd[b, g],  z = xhat * gamma[c] + beta[c],
//   out = act(scale * sum_{i < nsrc} z_i)      nsrc 1 or 3 (the predictor's three-branch average), act none or ReLU
// with mean / biased variance per (sample, group) over HW x (C / G) values.  Only C = 128, G = 32 is built: four channels per group,
// so one 16-byte lane load covers two groups in bf16 and one in fp32.
//
// Work split: a block of 256 threads owns one chunk of 256 pixels of one sample; C / CE lanes side by side cover a pixel (16 in bf16,
// 32 in fp32), the rows of lanes sweep the chunk's pixels.  Every operand is (B * HW) pixels at an explicit pixel stride.
//
// Forward statistics: per chunk and group, two passes over the chunk (the second comes from cache): mean = K + sum(x - K) / n with K = x of
// the chunk's first pixel at the group's first channel (a sample of the data: |x - K| is of the order of the spread, not of the mean),
// then M2 = sum (x - mean)^2 - no difference of two large sums anywhere.  The consumer (apply) folds the chunks of its sample in chunk
// order with Chan's merge in its prologue: no finalize launch, no E[x^2] - E[x]^2, no atomics - the same bits on every run.
//
// Backward, given dz (gradient wrt out); the ReLU mask is recomputed from y, the bias and the saved statistics (no mask tensor):
//   dzh = dz * scale * mask,   per (b, g): s1 = sum dzh gamma, s2 = sum dzh gamma xhat,   n = HW * C / G
//   dy = rstd (dzh gamma - (s1 + xhat s2) / n)
//   dgamma[c] = sum_{b,p} dzh xhat,  dbeta[c] = sum_{b,p} dzh,
//   db_conv[c] = sum_{b,p} dy = sum_b rstd (gamma[c] dbeta_b[c] - (HW s1 + s2 sum_p xhat[c]) / n)       (the closed form of the sum)
// as a reduce pass (per chunk and channel: sum dzh xhat per source, sum xhat per source, sum dzh) and an apply pass whose prologue
// folds the chunks of its sample in chunk order; one extra block of the apply pass folds all samples into the parameter gradients.
//
// This file also holds the two small device passes of the predictor's tail: a two-stage per-channel column sum (the classifier's bias
// gradient) and the softmax expectation over the depth bins (`weighted_depth`).
#include "common.h"

namespace {

constexpr int GN_C = 128, GN_G = 32, GN_CPG = GN_C / GN_G, GN_T = 256, GN_CHUNK = 256, GN_MAXSRC = 3;

struct GnSrc {
  const void* y;      // raw conv output, (B * HW) pixels of GN_C channels at pixel stride sw
  long sw;
  const float* b;     // conv bias, gamma, beta: GN_C floats each
  const float* gamma;
  const float* beta;
  void* dy;           // backward apply: gradient wrt y at pixel stride dsw
  long dsw;
};
struct GnTab { GnSrc s[GN_MAXSRC]; };

template <typename T> struct GnGeo {
  static constexpr int CE = TT<T>::CE;
  static constexpr int LPP = GN_C / CE;    // lanes per pixel: 16 (bf16) / 32 (fp32)
  static constexpr int PPI = GN_T / LPP;   // pixels per sweep of the block: 16 / 8
  static constexpr int GPL = CE / GN_CPG;  // groups per lane: 2 / 1
};

__device__ __forceinline__ int gn_chunk_pixels(int HW, int chunk) {
  const int left = HW - chunk * GN_CHUNK;
  return left < GN_CHUNK ? left : GN_CHUNK;
}

// ---- forward statistics ----------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(GN_T) void gn_stats_kernel(GnTab tab, int B, int HW, int nchunk, float* __restrict__ part) {
  using Geo = GnGeo<T>;
  constexpr int CE = Geo::CE, LPP = Geo::LPP, PPI = Geo::PPI, GPL = Geo::GPL;
  __shared__ float sh[GN_T][GPL];
  __shared__ float gmean[GN_G];
  const int src = blockIdx.z, b = blockIdx.y, chunk = blockIdx.x;
  // (a select per field: indexing the by-value table with a run-time index would move it to scratch)
  const T* y = (const T*)(src == 0 ? tab.s[0].y : src == 1 ? tab.s[1].y : tab.s[2].y);
  const long sw = src == 0 ? tab.s[0].sw : src == 1 ? tab.s[1].sw : tab.s[2].sw;
  const float* bc = src == 0 ? tab.s[0].b : src == 1 ? tab.s[1].b : tab.s[2].b;
  const int tid = threadIdx.x, lane = tid % LPP, row = tid / LPP;
  const int pn = gn_chunk_pixels(HW, chunk);
  const T* base = y + ((long)b * HW + (long)chunk * GN_CHUNK) * sw;
  float bias[CE], K[GPL], acc[GPL];
#pragma unroll
  for (int e = 0; e < CE; ++e) bias[e] = bc[lane * CE + e];
#pragma unroll
  for (int q = 0; q < GPL; ++q) {
    K[q] = TT<T>::ld(base + lane * CE + q * GN_CPG) + bias[q * GN_CPG];
    acc[q] = 0.f;
  }
  const float n = (float)(pn * GN_CPG);
  // pass 1: the chunk's mean per group, as K + sum(x - K) / n
  for (int p = row; p < pn; p += PPI) {
    float f[CE];
    Chunk<T>::unpack(*reinterpret_cast<const uint4*>(base + (long)p * sw + lane * CE), f);
#pragma unroll
    for (int e = 0; e < CE; ++e) acc[e / GN_CPG] += (f[e] + bias[e]) - K[e / GN_CPG];
  }
#pragma unroll
  for (int q = 0; q < GPL; ++q) sh[tid][q] = acc[q];
  __syncthreads();
  if (tid < GN_G) {
    const int g = tid, ol = g / GPL, q = g % GPL;
    float a = 0.f;
    for (int r = 0; r < PPI; ++r) a += sh[r * LPP + ol][q];  // the rows of lanes in a fixed order
    const float Kg = TT<T>::ld(base + g * GN_CPG) + bc[g * GN_CPG];
    gmean[g] = Kg + a / n;
  }
  __syncthreads();
  // pass 2 (the chunk comes from cache): M2 = sum (x - mean)^2
  float mean[GPL];
#pragma unroll
  for (int q = 0; q < GPL; ++q) {
    mean[q] = gmean[lane * GPL + q];
    acc[q] = 0.f;
  }
  for (int p = row; p < pn; p += PPI) {
    float f[CE];
    Chunk<T>::unpack(*reinterpret_cast<const uint4*>(base + (long)p * sw + lane * CE), f);
#pragma unroll
    for (int e = 0; e < CE; ++e) {
      const float d = (f[e] + bias[e]) - mean[e / GN_CPG];
      acc[e / GN_CPG] += d * d;
    }
  }
#pragma unroll
  for (int q = 0; q < GPL; ++q) sh[tid][q] = acc[q];
  __syncthreads();
  if (tid < GN_G) {
    const int g = tid, ol = g / GPL, q = g % GPL;
    float a = 0.f;
    for (int r = 0; r < PPI; ++r) a += sh[r * LPP + ol][q];
    float* o = part + ((((long)src * B + b) * nchunk + chunk) * GN_G + g) * 2;
    o[0] = gmean[g];
    o[1] = a;
  }
}

// threads 0 .. nsrc * GN_G - 1: the chunk partials of (source, sample b, group) merged in chunk order (Chan) -> mr[src][g] = (mean, rstd)
template <int NSRC>
__device__ __forceinline__ void gn_fold_stats(const float* __restrict__ part, int B, int b, int HW, int nchunk, float eps, float (*mr)[GN_G][2]) {
  const int t = threadIdx.x;
  if (t < NSRC * GN_G) {
    const int src = t / GN_G, g = t % GN_G;
    const float* p = part + (((long)src * B + b) * nchunk) * GN_G * 2 + g * 2;
    float n = 0.f, mean = 0.f, M2 = 0.f;
    for (int c = 0; c < nchunk; ++c) {
      const float nb = (float)(gn_chunk_pixels(HW, c) * GN_CPG), mb = p[(long)c * GN_G * 2], Mb = p[(long)c * GN_G * 2 + 1];
      const float nt = n + nb, delta = mb - mean;
      mean = mean + delta * (nb / nt);
      M2 = M2 + Mb + delta * delta * (n * nb / nt);
      n = nt;
    }
    mr[src][g][0] = mean;
    mr[src][g][1] = 1.f / sqrtf(M2 / n + eps);
  }
  __syncthreads();
}

// per-lane constants of one source: conv bias, gamma, beta of the lane's CE channels, (mean, rstd) of its GPL groups
template <typename T> struct GnLane {
  float bias[GnGeo<T>::CE], gamma[GnGeo<T>::CE], beta[GnGeo<T>::CE], mean[GnGeo<T>::GPL], rstd[GnGeo<T>::GPL];
  __device__ __forceinline__ void load(const GnSrc& s, int lane, const float (*mr)[2]) {
    constexpr int CE = GnGeo<T>::CE, GPL = GnGeo<T>::GPL;
#pragma unroll
    for (int e = 0; e < CE; ++e) {
      bias[e] = s.b[lane * CE + e];
      gamma[e] = s.gamma[lane * CE + e];
      beta[e] = s.beta[lane * CE + e];
    }
#pragma unroll
    for (int q = 0; q < GPL; ++q) {
      mean[q] = mr[lane * GPL + q][0];
      rstd[q] = mr[lane * GPL + q][1];
    }
  }
};

// the pixel's xhat per source and its pre-activation v = scale * sum_i z_i: ONE formula for the forward and for the mask of the backward
template <typename T, int NSRC>
__device__ __forceinline__ void gn_pixel(const GnTab& tab, const GnLane<T>* L, long pix, int lane, float scale, float (*xhat)[GnGeo<T>::CE],
                                         float* v) {
  constexpr int CE = GnGeo<T>::CE;
#pragma unroll
  for (int i = 0; i < NSRC; ++i) {
    float f[CE];
    Chunk<T>::unpack(*reinterpret_cast<const uint4*>((const T*)tab.s[i].y + pix * tab.s[i].sw + lane * CE), f);
#pragma unroll
    for (int e = 0; e < CE; ++e) {
      const float x = f[e] + L[i].bias[e];
      xhat[i][e] = (x - L[i].mean[e / GN_CPG]) * L[i].rstd[e / GN_CPG];
      const float z = xhat[i][e] * L[i].gamma[e] + L[i].beta[e];
      v[e] = i == 0 ? z : v[e] + z;
    }
  }
#pragma unroll
  for (int e = 0; e < CE; ++e) v[e] = v[e] * scale;
}

// ---- forward apply ---------------------------------------------------------------------------------------------------------------
template <typename T, int NSRC, bool RELU>
__global__ __launch_bounds__(GN_T) void gn_apply_kernel(GnTab tab, const float* __restrict__ part, float eps, float scale, T* __restrict__ out,
                                                        long osw, float* __restrict__ stats, int B, int HW, int nchunk) {
  using Geo = GnGeo<T>;
  constexpr int CE = Geo::CE, LPP = Geo::LPP, PPI = Geo::PPI;
  __shared__ float mr[NSRC][GN_G][2];
  const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x, lane = tid % LPP, row = tid / LPP;
  gn_fold_stats<NSRC>(part, B, b, HW, nchunk, eps, mr);
  if (chunk == 0 && tid < NSRC * GN_G) {  // saved for the backward: [src][B][G](mean, rstd)
    const int src = tid / GN_G, g = tid % GN_G;
    float* o = stats + (((long)src * B + b) * GN_G + g) * 2;
    o[0] = mr[src][g][0];
    o[1] = mr[src][g][1];
  }
  GnLane<T> L[NSRC];
#pragma unroll
  for (int i = 0; i < NSRC; ++i) L[i].load(tab.s[i], lane, mr[i]);
  const int pn = gn_chunk_pixels(HW, chunk);
  const long pix0 = (long)b * HW + (long)chunk * GN_CHUNK;
  for (int p = row; p < pn; p += PPI) {
    float xhat[NSRC][CE], v[CE];
    gn_pixel<T, NSRC>(tab, L, pix0 + p, lane, scale, xhat, v);
    if (RELU) {
#pragma unroll
      for (int e = 0; e < CE; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
    }
    *reinterpret_cast<uint4*>(out + (pix0 + p) * osw + lane * CE) = Chunk<T>::pack(v);
  }
}

// ---- backward reduce -------------------------------------------------------------------------------------------------------------
// bpart[b][chunk][q][GN_C], q = i: sum dzh xhat_i, NSRC + i: sum xhat_i, 2 NSRC: sum dzh
template <typename T, int NSRC, bool RELU>
__global__ __launch_bounds__(GN_T) void gn_bwd_reduce_kernel(GnTab tab, const float* __restrict__ stats, float scale, const T* __restrict__ dz,
                                                             long dsw, float* __restrict__ bpart, int B, int HW, int nchunk) {
  using Geo = GnGeo<T>;
  constexpr int CE = Geo::CE, LPP = Geo::LPP, PPI = Geo::PPI, NQ = 2 * NSRC + 1;
  __shared__ float sh[PPI][GN_C];
  const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x, lane = tid % LPP, row = tid / LPP;
  GnLane<T> L[NSRC];
#pragma unroll
  for (int i = 0; i < NSRC; ++i) L[i].load(tab.s[i], lane, reinterpret_cast<const float(*)[2]>(stats + ((long)i * B + b) * GN_G * 2));
  float acc[NQ][CE];
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int e = 0; e < CE; ++e) acc[q][e] = 0.f;
  const int pn = gn_chunk_pixels(HW, chunk);
  const long pix0 = (long)b * HW + (long)chunk * GN_CHUNK;
  for (int p = row; p < pn; p += PPI) {
    float xhat[NSRC][CE], v[CE], g[CE];
    gn_pixel<T, NSRC>(tab, L, pix0 + p, lane, scale, xhat, v);
    Chunk<T>::unpack(*reinterpret_cast<const uint4*>(dz + (pix0 + p) * dsw + lane * CE), g);
#pragma unroll
    for (int e = 0; e < CE; ++e) {
      const float dzh = (!RELU || v[e] > 0.f) ? g[e] * scale : 0.f;
#pragma unroll
      for (int i = 0; i < NSRC; ++i) {
        acc[i][e] += dzh * xhat[i][e];
        acc[NSRC + i][e] += xhat[i][e];
      }
      acc[2 * NSRC][e] += dzh;
    }
  }
  float* o = bpart + (((long)b * nchunk + chunk) * NQ) * GN_C;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
#pragma unroll
    for (int e = 0; e < CE; ++e) sh[row][lane * CE + e] = acc[q][e];
    __syncthreads();
    if (tid < GN_C) {
      float a = 0.f;
      for (int r = 0; r < PPI; ++r) a += sh[r][tid];  // the rows of lanes in a fixed order
      o[q * GN_C + tid] = a;
    }
    __syncthreads();
  }
}

// ---- backward apply --------------------------------------------------------------------------------------------------------------
// the chunk partials of sample b folded in chunk order -> tot[q][c]; then per (source, group) s12 = (s1, s2)
template <int NSRC>
__device__ __forceinline__ void gn_fold_bwd(const GnTab& tab, const float* __restrict__ bpart, int b, int nchunk, float (*tot)[GN_C],
                                            float (*s12)[GN_G][2]) {
  constexpr int NQ = 2 * NSRC + 1;
  const int t = threadIdx.x;
  if (t < GN_C) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      float a = 0.f;
      for (int c = 0; c < nchunk; ++c) a += bpart[(((long)b * nchunk + c) * NQ + q) * GN_C + t];
      tot[q][t] = a;
    }
  }
  __syncthreads();
  if (t < NSRC * GN_G) {
    const int g = t % GN_G;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NSRC; ++i) {
      if (i == t / GN_G) {
#pragma unroll
        for (int k = 0; k < GN_CPG; ++k) {
          const float gm = tab.s[i].gamma[g * GN_CPG + k];
          s1 += gm * tot[2 * NSRC][g * GN_CPG + k];
          s2 += gm * tot[i][g * GN_CPG + k];
        }
        s12[i][g][0] = s1;
        s12[i][g][1] = s2;
      }
    }
  }
  __syncthreads();
}

// grid (nchunk, B + 1): rows 0 .. B - 1 write dy of their chunk; block (0, B) folds every sample into dgamma / dbeta / db_conv [src][GN_C]
template <typename T, int NSRC, bool RELU>
__global__ __launch_bounds__(GN_T) void gn_bwd_apply_kernel(GnTab tab, const float* __restrict__ stats, float scale, const T* __restrict__ dz,
                                                            long dsw, const float* __restrict__ bpart, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, float* __restrict__ dbconv, int B, int HW, int nchunk) {
  using Geo = GnGeo<T>;
  constexpr int CE = Geo::CE, LPP = Geo::LPP, PPI = Geo::PPI, GPL = Geo::GPL, NQ = 2 * NSRC + 1;
  __shared__ float tot[NQ][GN_C];
  __shared__ float s12[NSRC][GN_G][2];
  const int tid = threadIdx.x;
  const float n = (float)HW * (float)GN_CPG;
  if ((int)blockIdx.y == B) {
    if (blockIdx.x != 0) return;
    float dg[NSRC], dbc[NSRC], db = 0.f;
#pragma unroll
    for (int i = 0; i < NSRC; ++i) dg[i] = dbc[i] = 0.f;
    for (int b = 0; b < B; ++b) {  // the samples in a fixed order
      gn_fold_bwd<NSRC>(tab, bpart, b, nchunk, tot, s12);
      if (tid < GN_C) {
        const int g = tid / GN_CPG;
        db += tot[2 * NSRC][tid];
#pragma unroll
        for (int i = 0; i < NSRC; ++i) {
          const float rstd = stats[(((long)i * B + b) * GN_G + g) * 2 + 1];
          dg[i] += tot[i][tid];
          dbc[i] += rstd * (tab.s[i].gamma[tid] * tot[2 * NSRC][tid] - ((float)HW * s12[i][g][0] + s12[i][g][1] * tot[NSRC + i][tid]) / n);
        }
      }
      __syncthreads();  // tot / s12 are rewritten by the next sample
    }
    if (tid < GN_C) {
#pragma unroll
      for (int i = 0; i < NSRC; ++i) {
        dgamma[i * GN_C + tid] = dg[i];
        dbeta[i * GN_C + tid] = db;
        dbconv[i * GN_C + tid] = dbc[i];
      }
    }
    return;
  }
  const int b = blockIdx.y, chunk = blockIdx.x, lane = tid % LPP, row = tid / LPP;
  gn_fold_bwd<NSRC>(tab, bpart, b, nchunk, tot, s12);
  GnLane<T> L[NSRC];
  float s1[NSRC][GPL], s2[NSRC][GPL];
#pragma unroll
  for (int i = 0; i < NSRC; ++i) {
    L[i].load(tab.s[i], lane, reinterpret_cast<const float(*)[2]>(stats + ((long)i * B + b) * GN_G * 2));
#pragma unroll
    for (int q = 0; q < GPL; ++q) {
      s1[i][q] = s12[i][lane * GPL + q][0];
      s2[i][q] = s12[i][lane * GPL + q][1];
    }
  }
  const int pn = gn_chunk_pixels(HW, chunk);
  const long pix0 = (long)b * HW + (long)chunk * GN_CHUNK;
  for (int p = row; p < pn; p += PPI) {
    float xhat[NSRC][CE], v[CE], g[CE];
    gn_pixel<T, NSRC>(tab, L, pix0 + p, lane, scale, xhat, v);
    Chunk<T>::unpack(*reinterpret_cast<const uint4*>(dz + (pix0 + p) * dsw + lane * CE), g);
#pragma unroll
    for (int i = 0; i < NSRC; ++i) {
      float d[CE];
#pragma unroll
      for (int e = 0; e < CE; ++e) {
        const float dzh = (!RELU || v[e] > 0.f) ? g[e] * scale : 0.f;
        const int q = e / GN_CPG;
        // (+ 0.f: a -0 product of a zero dzh and a negative gamma leaves as +0)
        d[e] = L[i].rstd[q] * (dzh * L[i].gamma[e] - (s1[i][q] + xhat[i][e] * s2[i][q]) / n) + 0.f;
      }
      *reinterpret_cast<uint4*>((T*)tab.s[i].dy + (pix0 + p) * tab.s[i].dsw + lane * CE) = Chunk<T>::pack(d);
    }
  }
}

// ---- per-channel column sum over pixels, two stages in a fixed order ----------------------------------------------------------------
constexpr int CS_CHUNK = 1024, CS_CMAX = 256;

template <typename T>
__global__ __launch_bounds__(GN_T) void colsum_part_kernel(const T* __restrict__ x, long sw, long M, int C, float* __restrict__ part) {
  constexpr int CE = TT<T>::CE;
  __shared__ float sh[GN_T * CE];  // [row][C], rows * C <= 256 * CE
  const int lpp = C / CE, ppi = GN_T / lpp, tid = threadIdx.x, lane = tid % lpp, row = tid / lpp;
  const long p0 = (long)blockIdx.x * CS_CHUNK;
  const int pn = (int)(M - p0 < CS_CHUNK ? M - p0 : CS_CHUNK);
  float acc[CE];
#pragma unroll
  for (int e = 0; e < CE; ++e) acc[e] = 0.f;
  if (row < ppi) {
    for (int p = row; p < pn; p += ppi) {
      float f[CE];
      Chunk<T>::unpack(*reinterpret_cast<const uint4*>(x + (p0 + p) * sw + lane * CE), f);
#pragma unroll
      for (int e = 0; e < CE; ++e) acc[e] += f[e];
    }
#pragma unroll
    for (int e = 0; e < CE; ++e) sh[row * C + lane * CE + e] = acc[e];
  }
  __syncthreads();
  if (tid < C) {
    float a = 0.f;
    for (int r = 0; r < ppi; ++r) a += sh[r * C + tid];
    part[(long)blockIdx.x * C + tid] = a;
  }
}

__global__ __launch_bounds__(CS_CMAX) void colsum_fold_kernel(const float* __restrict__ part, int nblk, int C, float* __restrict__ out) {
  const int t = threadIdx.x;
  if (t < C) {
    float a = 0.f;
    for (int i = 0; i < nblk; ++i) a += part[(long)i * C + t];
    out[t] = a;
  }
}

// ---- weighted depth: sum_c softmax(logits)_c * bins[c], one thread per cell ---------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(GN_T) void depth_expect_kernel(const T* __restrict__ z, long sw, long M, int C, const float* __restrict__ bins,
                                                            float* __restrict__ out) {
  constexpr int CE = TT<T>::CE;
  const long cell = (long)blockIdx.x * GN_T + threadIdx.x;
  if (cell >= M) return;
  const T* zp = z + cell * sw;
  const int nk = (C + CE - 1) / CE;  // the row is sw >= nk * CE elements long: whole 16-byte pieces, the tail masked by channel
  float m = -INFINITY;
  for (int k = 0; k < nk; ++k) {
    float f[CE];
    Chunk<T>::unpack(*reinterpret_cast<const uint4*>(zp + k * CE), f);
#pragma unroll
    for (int e = 0; e < CE; ++e)
      if (k * CE + e < C) m = fmaxf(m, f[e]);
  }
  float s = 0.f, w = 0.f;
  for (int k = 0; k < nk; ++k) {
    float f[CE];
    Chunk<T>::unpack(*reinterpret_cast<const uint4*>(zp + k * CE), f);
#pragma unroll
    for (int e = 0; e < CE; ++e)
      if (k * CE + e < C) {
        const float ex = expf(f[e] - m);
        s += ex;
        w += ex * bins[k * CE + e];
      }
  }
  out[cell] = w / s;
}

int gn_check(const char* who, int dtype, int nsrc, const void* const* y, const int64_t* ysw, const float* const* bconv, int B, int HW, int C, int G) {
  Y3D_CHECK(dtype == Y3D_BF16 || dtype == Y3D_F32, "%s: bad dtype", who);
  const int ce = dtype == Y3D_BF16 ? 8 : 4;
  Y3D_CHECK(C % ce == 0, "%s: C = %d is no whole number of 16-byte chunks (%d channels each)", who, C, ce);
  Y3D_CHECK(C == GN_C && G == GN_G, "%s: only GroupNorm(%d groups, %d channels) is built (got %d groups, %d channels)", who, GN_G, GN_C, G, C);
  Y3D_CHECK(nsrc == 1 || nsrc == GN_MAXSRC, "%s: nsrc = %d: 1 or %d", who, nsrc, GN_MAXSRC);
  Y3D_CHECK(B >= 1 && HW >= 1 && (long)B * HW < (1L << 31), "%s: B >= 1, HW >= 1, B * HW < 2^31", who);
  Y3D_CHECK(y != nullptr && ysw != nullptr && bconv != nullptr, "%s: null table", who);
  for (int i = 0; i < nsrc; ++i) {
    Y3D_CHECK(y[i] != nullptr && bconv[i] != nullptr, "%s: null pointer in source %d", who, i);
    Y3D_CHECK((uintptr_t)y[i] % 16 == 0 && ysw[i] >= C && ysw[i] % ce == 0, "%s: source %d must be 16-byte aligned with a pixel stride >= C in whole chunks", who, i);
  }
  return Y3D_OK;
}

GnTab gn_table(int nsrc, const void* const* y, const int64_t* ysw, const float* const* bconv, const float* const* gamma, const float* const* beta,
               void* const* dy, const int64_t* dysw) {
  GnTab t;
  for (int i = 0; i < GN_MAXSRC; ++i) {
    const int j = i < nsrc ? i : 0;  // unused slots repeat source 0: never read
    t.s[i].y = y[j];
    t.s[i].sw = (long)ysw[j];
    t.s[i].b = bconv[j];
    t.s[i].gamma = gamma ? gamma[j] : nullptr;
    t.s[i].beta = beta ? beta[j] : nullptr;
    t.s[i].dy = dy ? dy[j] : nullptr;
    t.s[i].dsw = dysw ? (long)dysw[j] : 0;
  }
  return t;
}

}  // namespace

extern "C" {

int y3d_gn_chunks(int HW) { return HW < 1 ? 0 : cdiv(HW, GN_CHUNK); }

int y3d_gn_stats(int dtype, int nsrc, const void* const* y, const int64_t* ysw, const float* const* bconv, int B, int HW, int C, int G,
                 float* partials, void* stream) {
  if (int rc = gn_check("gn_stats", dtype, nsrc, y, ysw, bconv, B, HW, C, G)) return rc;
  Y3D_CHECK(partials != nullptr, "gn_stats: null partials");
  Y3D_CHECK(B <= 65535, "gn_stats: B <= 65535");
  const int nchunk = cdiv(HW, GN_CHUNK);
  const GnTab tab = gn_table(nsrc, y, ysw, bconv, nullptr, nullptr, nullptr, nullptr);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == Y3D_BF16) hipLaunchKernelGGL(gn_stats_kernel<bf16_t>, dim3(nchunk, B, nsrc), dim3(GN_T), 0, st, tab, B, HW, nchunk, partials);
  else hipLaunchKernelGGL(gn_stats_kernel<float>, dim3(nchunk, B, nsrc), dim3(GN_T), 0, st, tab, B, HW, nchunk, partials);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_gn_apply(int dtype, int nsrc, const void* const* y, const int64_t* ysw, const float* const* bconv, const float* const* gamma,
                 const float* const* beta, const float* partials, float eps, float scale, int relu, void* out, int64_t osw, float* stats, int B,
                 int HW, int C, int G, void* stream) {
  if (int rc = gn_check("gn_apply", dtype, nsrc, y, ysw, bconv, B, HW, C, G)) return rc;
  const int ce = dtype == Y3D_BF16 ? 8 : 4;
  Y3D_CHECK(gamma != nullptr && beta != nullptr && partials != nullptr && out != nullptr && stats != nullptr, "gn_apply: null pointer");
  for (int i = 0; i < nsrc; ++i) Y3D_CHECK(gamma[i] != nullptr && beta[i] != nullptr, "gn_apply: null gamma / beta of source %d", i);
  Y3D_CHECK((uintptr_t)out % 16 == 0 && osw >= C && osw % ce == 0, "gn_apply: out must be 16-byte aligned with a pixel stride >= C in whole chunks");
  Y3D_CHECK(eps >= 0.f && B <= 65535, "gn_apply: eps >= 0, B <= 65535");
  const int nchunk = cdiv(HW, GN_CHUNK);
  const GnTab tab = gn_table(nsrc, y, ysw, bconv, gamma, beta, nullptr, nullptr);
  hipStream_t st = (hipStream_t)stream;
#define GN_ARGS(T) tab, partials, eps, scale, (T*)out, (long)osw, stats, B, HW, nchunk
  if (dtype == Y3D_BF16) {
    if (nsrc == 1) { if (relu) hipLaunchKernelGGL((gn_apply_kernel<bf16_t, 1, true>), dim3(nchunk, B), dim3(GN_T), 0, st, GN_ARGS(bf16_t));
                     else hipLaunchKernelGGL((gn_apply_kernel<bf16_t, 1, false>), dim3(nchunk, B), dim3(GN_T), 0, st, GN_ARGS(bf16_t)); }
    else { if (relu) hipLaunchKernelGGL((gn_apply_kernel<bf16_t, 3, true>), dim3(nchunk, B), dim3(GN_T), 0, st, GN_ARGS(bf16_t));
           else hipLaunchKernelGGL((gn_apply_kernel<bf16_t, 3, false>), dim3(nchunk, B), dim3(GN_T), 0, st, GN_ARGS(bf16_t)); }
  } else {
    if (nsrc == 1) { if (relu) hipLaunchKernelGGL((gn_apply_kernel<float, 1, true>), dim3(nchunk, B), dim3(GN_T), 0, st, GN_ARGS(float));
                     else hipLaunchKernelGGL((gn_apply_kernel<float, 1, false>), dim3(nchunk, B), dim3(GN_T), 0, st, GN_ARGS(float)); }
    else { if (relu) hipLaunchKernelGGL((gn_apply_kernel<float, 3, true>), dim3(nchunk, B), dim3(GN_T), 0, st, GN_ARGS(float));
           else hipLaunchKernelGGL((gn_apply_kernel<float, 3, false>), dim3(nchunk, B), dim3(GN_T), 0, st, GN_ARGS(float)); }
  }
#undef GN_ARGS
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

static int gn_bwd_check(const char* who, int dtype, int nsrc, const float* const* gamma, const float* const* beta, const float* stats, const void* dz,
                        int64_t dsw, const float* partials, int C, int B) {
  const int ce = dtype == Y3D_BF16 ? 8 : 4;
  Y3D_CHECK(gamma != nullptr && beta != nullptr && stats != nullptr && dz != nullptr && partials != nullptr, "%s: null pointer", who);
  for (int i = 0; i < nsrc; ++i) Y3D_CHECK(gamma[i] != nullptr && beta[i] != nullptr, "%s: null gamma / beta of source %d", who, i);
  Y3D_CHECK((uintptr_t)dz % 16 == 0 && dsw >= C && dsw % ce == 0, "%s: dz must be 16-byte aligned with a pixel stride >= C in whole chunks", who);
  Y3D_CHECK(B < 65535, "%s: B < 65535", who);
  return Y3D_OK;
}

int y3d_gn_bwd_reduce(int dtype, int nsrc, const void* const* y, const int64_t* ysw, const float* const* bconv, const float* const* gamma,
                      const float* const* beta, const float* stats, float scale, int relu, const void* dz, int64_t dsw, float* partials, int B,
                      int HW, int C, int G, void* stream) {
  if (int rc = gn_check("gn_bwd_reduce", dtype, nsrc, y, ysw, bconv, B, HW, C, G)) return rc;
  if (int rc = gn_bwd_check("gn_bwd_reduce", dtype, nsrc, gamma, beta, stats, dz, dsw, partials, C, B)) return rc;
  const int nchunk = cdiv(HW, GN_CHUNK);
  const GnTab tab = gn_table(nsrc, y, ysw, bconv, gamma, beta, nullptr, nullptr);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == Y3D_BF16) {
#define GN_ARGS tab, stats, scale, (const bf16_t*)dz, (long)dsw, partials, B, HW, nchunk
    if (nsrc == 1) { if (relu) hipLaunchKernelGGL((gn_bwd_reduce_kernel<bf16_t, 1, true>), dim3(nchunk, B), dim3(GN_T), 0, st, GN_ARGS);
                     else hipLaunchKernelGGL((gn_bwd_reduce_kernel<bf16_t, 1, false>), dim3(nchunk, B), dim3(GN_T), 0, st, GN_ARGS); }
    else { if (relu) hipLaunchKernelGGL((gn_bwd_reduce_kernel<bf16_t, 3, true>), dim3(nchunk, B), dim3(GN_T), 0, st, GN_ARGS);
           else hipLaunchKernelGGL((gn_bwd_reduce_kernel<bf16_t, 3, false>), dim3(nchunk, B), dim3(GN_T), 0, st, GN_ARGS); }
#undef GN_ARGS
  } else {
#define GN_ARGS tab, stats, scale, (const float*)dz, (long)dsw, partials, B, HW, nchunk
    if (nsrc == 1) { if (relu) hipLaunchKernelGGL((gn_bwd_reduce_kernel<float, 1, true>), dim3(nchunk, B), dim3(GN_T), 0, st, GN_ARGS);
                     else hipLaunchKernelGGL((gn_bwd_reduce_kernel<float, 1, false>), dim3(nchunk, B), dim3(GN_T), 0, st, GN_ARGS); }
    else { if (relu) hipLaunchKernelGGL((gn_bwd_reduce_kernel<float, 3, true>), dim3(nchunk, B), dim3(GN_T), 0, st, GN_ARGS);
           else hipLaunchKernelGGL((gn_bwd_reduce_kernel<float, 3, false>), dim3(nchunk, B), dim3(GN_T), 0, st, GN_ARGS); }
#undef GN_ARGS
  }
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_gn_bwd_apply(int dtype, int nsrc, const void* const* y, const int64_t* ysw, const float* const* bconv, const float* const* gamma,
                     const float* const* beta, const float* stats, float scale, int relu, const void* dz, int64_t dsw, const float* partials,
                     void* const* dy, const int64_t* dysw, float* dgamma, float* dbeta, float* dbconv, int B, int HW, int C, int G, void* stream) {
  if (int rc = gn_check("gn_bwd_apply", dtype, nsrc, y, ysw, bconv, B, HW, C, G)) return rc;
  if (int rc = gn_bwd_check("gn_bwd_apply", dtype, nsrc, gamma, beta, stats, dz, dsw, partials, C, B)) return rc;
  const int ce = dtype == Y3D_BF16 ? 8 : 4;
  Y3D_CHECK(dy != nullptr && dysw != nullptr && dgamma != nullptr && dbeta != nullptr && dbconv != nullptr, "gn_bwd_apply: null pointer");
  for (int i = 0; i < nsrc; ++i)
    Y3D_CHECK(dy[i] != nullptr && (uintptr_t)dy[i] % 16 == 0 && dysw[i] >= C && dysw[i] % ce == 0,
              "gn_bwd_apply: dy of source %d must be 16-byte aligned with a pixel stride >= C in whole chunks", i);
  const int nchunk = cdiv(HW, GN_CHUNK);
  const GnTab tab = gn_table(nsrc, y, ysw, bconv, gamma, beta, dy, dysw);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == Y3D_BF16) {
#define GN_ARGS tab, stats, scale, (const bf16_t*)dz, (long)dsw, partials, dgamma, dbeta, dbconv, B, HW, nchunk
    if (nsrc == 1) { if (relu) hipLaunchKernelGGL((gn_bwd_apply_kernel<bf16_t, 1, true>), dim3(nchunk, B + 1), dim3(GN_T), 0, st, GN_ARGS);
                     else hipLaunchKernelGGL((gn_bwd_apply_kernel<bf16_t, 1, false>), dim3(nchunk, B + 1), dim3(GN_T), 0, st, GN_ARGS); }
    else { if (relu) hipLaunchKernelGGL((gn_bwd_apply_kernel<bf16_t, 3, true>), dim3(nchunk, B + 1), dim3(GN_T), 0, st, GN_ARGS);
           else hipLaunchKernelGGL((gn_bwd_apply_kernel<bf16_t, 3, false>), dim3(nchunk, B + 1), dim3(GN_T), 0, st, GN_ARGS); }
#undef GN_ARGS
  } else {
#define GN_ARGS tab, stats, scale, (const float*)dz, (long)dsw, partials, dgamma, dbeta, dbconv, B, HW, nchunk
    if (nsrc == 1) { if (relu) hipLaunchKernelGGL((gn_bwd_apply_kernel<float, 1, true>), dim3(nchunk, B + 1), dim3(GN_T), 0, st, GN_ARGS);
                     else hipLaunchKernelGGL((gn_bwd_apply_kernel<float, 1, false>), dim3(nchunk, B + 1), dim3(GN_T), 0, st, GN_ARGS); }
    else { if (relu) hipLaunchKernelGGL((gn_bwd_apply_kernel<float, 3, true>), dim3(nchunk, B + 1), dim3(GN_T), 0, st, GN_ARGS);
           else hipLaunchKernelGGL((gn_bwd_apply_kernel<float, 3, false>), dim3(nchunk, B + 1), dim3(GN_T), 0, st, GN_ARGS); }
#undef GN_ARGS
  }
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_colsum_blocks(int64_t M) { return M < 1 ? 0 : cdiv((long)M, CS_CHUNK); }

int y3d_colsum(int dtype, const void* x, int64_t xsw, int64_t M, int C, float* partials, float* out, void* stream) {
  Y3D_CHECK(dtype == Y3D_BF16 || dtype == Y3D_F32, "colsum: bad dtype");
  const int ce = dtype == Y3D_BF16 ? 8 : 4;
  Y3D_CHECK(M >= 1 && C >= ce && C <= CS_CMAX && C % ce == 0, "colsum: M >= 1 and C = %d must be a multiple of %d in %d..%d", C, ce, ce, CS_CMAX);
  Y3D_CHECK(x != nullptr && partials != nullptr && out != nullptr, "colsum: null pointer");
  Y3D_CHECK((uintptr_t)x % 16 == 0 && xsw >= C && xsw % ce == 0, "colsum: x must be 16-byte aligned with a pixel stride >= C in whole chunks");
  const int nblk = cdiv((long)M, CS_CHUNK);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == Y3D_BF16) hipLaunchKernelGGL(colsum_part_kernel<bf16_t>, dim3(nblk), dim3(GN_T), 0, st, (const bf16_t*)x, (long)xsw, (long)M, C, partials);
  else hipLaunchKernelGGL(colsum_part_kernel<float>, dim3(nblk), dim3(GN_T), 0, st, (const float*)x, (long)xsw, (long)M, C, partials);
  hipLaunchKernelGGL(colsum_fold_kernel, dim3(1), dim3(CS_CMAX), 0, st, partials, nblk, C, out);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_depth_expect(int dtype, const void* logits, int64_t sw, int64_t M, int C, const float* bins, float* out, void* stream) {
  Y3D_CHECK(dtype == Y3D_BF16 || dtype == Y3D_F32, "depth_expect: bad dtype");
  const int ce = dtype == Y3D_BF16 ? 8 : 4;
  Y3D_CHECK(M >= 1 && C >= 1, "depth_expect: M >= 1, C >= 1");
  Y3D_CHECK(logits != nullptr && bins != nullptr && out != nullptr, "depth_expect: null pointer");
  Y3D_CHECK((uintptr_t)logits % 16 == 0 && sw % ce == 0 && sw >= (C + ce - 1) / ce * ce,
            "depth_expect: the logits' rows must be 16-byte aligned and hold the %d channels in whole 16-byte chunks", C);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == Y3D_BF16) hipLaunchKernelGGL(depth_expect_kernel<bf16_t>, dim3(cdiv((long)M, GN_T)), dim3(GN_T), 0, st, (const bf16_t*)logits, (long)sw, (long)M, C, bins, out);
  else hipLaunchKernelGGL(depth_expect_kernel<float>, dim3(cdiv((long)M, GN_T)), dim3(GN_T), 0, st, (const float*)logits, (long)sw, (long)M, C, bins, out);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

}  // extern "C"
