// Foreground depth map loss (`ForegroundDepthMapLoss`, utils/loss.py:1225-1365 with LogitFocalLoss / focal_loss / one_hot at
// :1399-1564): a focal classification loss of supplied depth logits (B, num_bins + 1, h, w) against the LID bin of the foreground
// depth map (B, H, W) sampled at the centre of every 16 x 16 cell, balanced 13 : 1 between foreground and background cells.
//
// Per cell (b, i, j) of the (h, w) = (H / 16, W / 16) grid:
//   d    = map[b][ni(i)][ni(j)], ni = ATen's nearest-exact index (torchvision Resize(NEAREST_EXACT)):
//          min((int)floorf((float)((dst + 0.5) * scale)), in - 1), scale = (float)in / out, the product in double as ATen writes it
//   t    = LID bin of d in float64: idx = -0.5 + 0.5 * sqrt(1 + 8 * (d - dmin) / bin); idx < 0, idx > num_bins or not finite (the
//          background, d = 0 below dmin, arrives here through the NaN of the root) -> class num_bins, else (int)idx
//   p    = softmax(z), lp = log_softmax(z), f_c = -alpha (1 - p_c)^gamma lp_c
//   cell = sum_c (delta_ct + 1e-6) f_c            (the + 1e-6 of the reference's one_hot stays, in value and in gradient)
//   loss = sum over cells of (d > 0 ? fg_weight : bg_weight) * cell / number of cells
//
// Gradient.  With w_c = delta_ct + 1e-6 and g_c = p_c f'(p_c) = -alpha [(1 - p_c)^gamma - gamma (1 - p_c)^(gamma - 1) p_c lp_c]
// (the form that stays finite at saturated logits: no division by p),
//   d cell / d z_k = w_k g_k - p_k S,  S = sum_c w_c g_c.
//
// One thread owns one cell; a block is one wave of 64 cells.  The logits are swept twice in memory: once in (each value lands in
// LDS as z - max, channel-major, so lane l reads bank l: no conflict), once out (the gradient, in the logits' dtype and strides).
// Between the two the sums (softmax denominator, then cell loss and S) run over the LDS copy; no softmax tensor exists in memory.
// Arithmetic is fp32 with IEEE division, expf, logf.  The 64 weighted cell losses of a block fold through the fixed DPP / row-swap
// tree of common.h into one partial; a second single-block launch folds the partials in a fixed order in double: the same bits on
// every run, no float atomics.
#include "common.h"

namespace {

constexpr int FG_CELLS = 64;   // cells (threads) per block: one wave
constexpr int FG_CMAX = 256;   // channels: FG_CMAX * FG_CELLS floats = the 64 KiB of LDS a block may ask for

__device__ __forceinline__ float fg_wave_sum(float v) { return lane_xor32_sum(lane_xor16_sum(wave_xor_sum16(v))); }

__device__ __forceinline__ int nearest_exact(int dst, int in, float scale) {
  const int s = (int)floorf((float)(((double)dst + 0.5) * (double)scale));
  return s < in - 1 ? s : in - 1;
}

// (1 - p)^gamma and gamma (1 - p)^(gamma - 1): gamma == 2 (the reference's value, torch.pow squares) without powf
__device__ __forceinline__ void focal_powers(float q, float gamma, float& qg, float& gq1) {
  if (gamma == 2.f) { qg = q * q; gq1 = 2.f * q; }
  else if (gamma == 0.f) { qg = 1.f; gq1 = 0.f; }
  else { qg = powf(q, gamma); gq1 = gamma * powf(q, gamma - 1.f); }
}

// T: logits / gradient dtype; TM: depth map dtype (float or double)
template <typename T, typename TM>
__global__ __launch_bounds__(FG_CELLS) void fgdm_loss_kernel(const T* __restrict__ z, long sb, long sc, long sh, long sw,
                                                             const TM* __restrict__ map, int B, int H, int W, int h, int w, int C,
                                                             double dmin, double bin, float alpha, float gamma, float fgw, float bgw,
                                                             T* __restrict__ dz, float* __restrict__ part, int* __restrict__ tgt) {
  extern __shared__ __attribute__((aligned(16))) float fg_lds[];  // [C][FG_CELLS]: z - max of the block's cells
  const int tid = threadIdx.x;
  const long ncell = (long)B * h * w;
  const long cell = (long)blockIdx.x * FG_CELLS + tid;
  float wl = 0.f;
  if (cell < ncell) {
    const int j = (int)(cell % w), i = (int)((cell / w) % h), b = (int)(cell / ((long)w * h));
    const int ys = nearest_exact(i, H, (float)H / (float)h), xs = nearest_exact(j, W, (float)W / (float)w);
    const TM dv = map[((long)b * H + ys) * W + xs];
    const double d = (double)dv;
    const double idx = -0.5 + 0.5 * sqrt(1.0 + 8.0 * (d - dmin) / bin);
    const int nb = C - 1;
    const int t = (idx < 0.0 || idx > (double)nb || !isfinite(idx)) ? nb : (int)idx;
    if (tgt != nullptr) tgt[cell] = t;
    const long base = (long)b * sb + (long)i * sh + (long)j * sw;
    const T* zp = z + base;
    // sweep in: logits -> LDS, running maximum
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) {
      const float v = TT<T>::ld(zp + (long)c * sc);
      fg_lds[c * FG_CELLS + tid] = v;
      m = fmaxf(m, v);
    }
    float s = 0.f;
    for (int c = 0; c < C; ++c) {
      const float zm = fg_lds[c * FG_CELLS + tid] - m;
      fg_lds[c * FG_CELLS + tid] = zm;
      s += expf(zm);
    }
    const float ls = logf(s);
    // cell loss and S = sum_c w_c g_c
    float lc = 0.f, S = 0.f;
    for (int c = 0; c < C; ++c) {
      const float zm = fg_lds[c * FG_CELLS + tid];
      const float p = expf(zm) / s, lp = zm - ls;
      float qg, gq1;
      focal_powers(1.f - p, gamma, qg, gq1);
      const float wc = (c == t ? 1.f : 0.f) + 1e-6f;
      lc += wc * (-alpha * qg * lp);
      S += wc * (-alpha * (qg - gq1 * p * lp));
    }
    const float wt = dv > (TM)0 ? fgw : bgw;
    wl = wt * lc;
    // sweep out: the gradient of the mean over cells
    const float coef = wt / (float)ncell;
    T* gp = dz + base;
    for (int c = 0; c < C; ++c) {
      const float zm = fg_lds[c * FG_CELLS + tid];
      const float p = expf(zm) / s, lp = zm - ls;
      float qg, gq1;
      focal_powers(1.f - p, gamma, qg, gq1);
      const float wc = (c == t ? 1.f : 0.f) + 1e-6f;
      const float g = -alpha * (qg - gq1 * p * lp);
      TT<T>::st(gp + (long)c * sc, coef * (wc * g - p * S));
    }
  }
  wl = fg_wave_sum(wl);  // cells past the end add +0
  if (tid == 0) part[blockIdx.x] = wl;
}

__global__ __launch_bounds__(256) void fgdm_fold_kernel(const float* __restrict__ part, int nblk, double ncell, float* __restrict__ loss) {
  __shared__ double sh[256];
  const int t = threadIdx.x;
  double a = 0.0;
  for (int i = t; i < nblk; i += 256) a += (double)part[i];
  sh[t] = a;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) sh[t] += sh[t + s];
    __syncthreads();
  }
  if (t == 0) loss[0] = (float)(sh[0] / ncell);
}

// dst[i] = src[i] * scale[0] over n elements of dense memory (any layout: the two share their strides), 16-byte pieces + a ragged end
template <typename T>
__global__ __launch_bounds__(256) void fgdm_scale_kernel(const T* __restrict__ src, const float* __restrict__ scale, T* __restrict__ dst, long n) {
  constexpr int CE = TT<T>::CE;
  const float s = scale[0];
  const long k = (long)blockIdx.x * 256 + threadIdx.x, nv = n / CE;
  if (k < nv) {
    float f[CE];
    Chunk<T>::unpack(reinterpret_cast<const uint4*>(src)[k], f);
#pragma unroll
    for (int e = 0; e < CE; ++e) f[e] = f[e] * s;
    reinterpret_cast<uint4*>(dst)[k] = Chunk<T>::pack(f);
  } else if (k - nv < n - nv * CE) {
    const long e = nv * CE + (k - nv);
    TT<T>::st(dst + e, TT<T>::ld(src + e) * s);
  }
}

}  // namespace

extern "C" {

int y3d_fgdm_loss_blocks(int B, int h, int w) {
  if (B < 1 || h < 1 || w < 1) return 0;
  return cdiv((long)B * h * w, FG_CELLS);
}

int y3d_fgdm_loss(int dtype, const void* logits, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int map_f64, const void* depth_map, int B,
                  int H, int W, int h, int w, int num_bins, double dmin, double dmax, float alpha, float gamma, float fg_weight,
                  float bg_weight, void* dlogits, float* partials, float* loss, int* targets, void* stream) {
  Y3D_CHECK(dtype == Y3D_BF16 || dtype == Y3D_F32, "fgdm_loss: bad dtype");
  Y3D_CHECK(B >= 1 && H >= 16 && W >= 16, "fgdm_loss: B >= 1 and a depth map of at least 16 x 16 (got %d x %d x %d)", B, H, W);
  Y3D_CHECK(h == H / 16 && w == W / 16, "fgdm_loss: the logits' grid %d x %d is not (H / 16, W / 16) = %d x %d", h, w, H / 16, W / 16);
  Y3D_CHECK(num_bins >= 1 && num_bins + 1 <= FG_CMAX, "fgdm_loss: num_bins = %d: 1..%d", num_bins, FG_CMAX - 1);
  Y3D_CHECK(dmax > dmin, "fgdm_loss: max_depth_threshold must exceed min_depth_threshold");
  Y3D_CHECK(gamma == 0.f || gamma >= 1.f, "fgdm_loss: gamma = %g: 0 or >= 1 (the gradient at p = 1 is not finite in between)", (double)gamma);
  Y3D_CHECK(sb >= 0 && sc >= 1 && sh >= 1 && sw >= 1, "fgdm_loss: the logits' strides must be positive");
  Y3D_CHECK(logits != nullptr && depth_map != nullptr && dlogits != nullptr && partials != nullptr && loss != nullptr, "fgdm_loss: null pointer");
  const int C = num_bins + 1;
  const double bin = 2.0 * (dmax - dmin) / ((double)num_bins * (1.0 + (double)num_bins));
  const long ncell = (long)B * h * w;
  const int nblk = cdiv(ncell, FG_CELLS);
  const size_t lds = (size_t)C * FG_CELLS * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
#define Y3D_FGDM(T, TM) hipLaunchKernelGGL((fgdm_loss_kernel<T, TM>), dim3(nblk), dim3(FG_CELLS), lds, st, (const T*)logits, (long)sb, (long)sc, \
                                           (long)sh, (long)sw, (const TM*)depth_map, B, H, W, h, w, C, dmin, bin, alpha, gamma, fg_weight,      \
                                           bg_weight, (T*)dlogits, partials, targets)
  if (dtype == Y3D_BF16) { if (map_f64) Y3D_FGDM(bf16_t, double); else Y3D_FGDM(bf16_t, float); }
  else { if (map_f64) Y3D_FGDM(float, double); else Y3D_FGDM(float, float); }
#undef Y3D_FGDM
  hipLaunchKernelGGL(fgdm_fold_kernel, dim3(1), dim3(256), 0, st, partials, nblk, (double)ncell, loss);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_fgdm_scale(int dtype, const void* src, const float* scale, void* dst, int64_t n, void* stream) {
  Y3D_CHECK(dtype == Y3D_BF16 || dtype == Y3D_F32, "fgdm_scale: bad dtype");
  Y3D_CHECK(n >= 1 && src != nullptr && dst != nullptr && scale != nullptr, "fgdm_scale: n >= 1 and non-null pointers");
  Y3D_CHECK((uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0, "fgdm_scale: 16-byte aligned buffers");
  const int ce = dtype == Y3D_BF16 ? 8 : 4;
  const long work = n / ce + n % ce;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == Y3D_BF16)
    hipLaunchKernelGGL(fgdm_scale_kernel<bf16_t>, dim3(cdiv(work, 256)), dim3(256), 0, st, (const bf16_t*)src, scale, (bf16_t*)dst, (long)n);
  else
    hipLaunchKernelGGL(fgdm_scale_kernel<float>, dim3(cdiv(work, 256)), dim3(256), 0, st, (const float*)src, scale, (float*)dst, (long)n);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

}  // extern "C"
