// Feature distillation of the 3D head (`distillation: True`): the seventh loss item `dis_om` / `dis_oo` and its gradient.
//
// Reference: utils/loss.py:1156-1188 SupervisionLoss.forward_head, called from DDDetectionLoss.__call__ (:893-898).  Per image the
// reference gathers the depth branch's first-layer embedding at every foreground anchor, gathers the teacher embedding at the
// projected 3D centre of the anchor's assigned object, and compares the two row sets with one of three criteria.  The teacher map
// is an INPUT here (any (B, C, h, w) tensor): the DINOv2 network that makes it in the reference is outside this library.
//
// The work is a few thousand rows of 64-128 channels: latency-bound.  One wave owns one foreground row; a lane owns chunks of four
// channels (8-byte loads of bf16, 16-byte loads of fp32), the softmax / norm sums cross the wave in registers, arithmetic is fp32.
// Nothing that reaches the loss or the gradient goes through a float atomic: the foreground anchors are compacted in (image,
// anchor) order by a block-wide scan, every row's loss goes to a per-block partial and one block folds the partials in a fixed
// order, so a replayed hipGraph reproduces the eager step bit for bit.
//
// Stages (one head set per call):
//   count    (one block per image)   participation of the image and its number of foreground anchors
//   index    (one block per image)   ordered compaction: row r -> (image, anchor); number of rows
//   rows     (one wave per row)      loss of the row -> block partial; gradient row (compute dtype)
//   final    (one block)             loss word = fixed-order sum of the partials
//   scatter  (one wave per row)      adds scale * row into a level's NHWC gradient map at the row's pixel (separate entry point)
//
// Two places where the reference is fragile, decided here:
//   * An image with valid objects but NO foreground anchor is 0/0 = NaN in the reference (the mean over an empty row set).  Here such
//     an image contributes 0: it has no rows, and nothing divides by its count.
//   * The reference indexes the list of an image's VALID objects with target_gt_idx, which indexes the padded rows.  The two agree
//     when the valid rows are a prefix of the padded rows, which y3d_pad_targets guarantees; the kernel reads padded row
//     target_gt_idx directly and relies on that.
#include "common.h"

namespace {

constexpr int DMAXL = 4;   // levels
constexpr int DKMAX = 4;   // 4-channel chunks per lane: C <= 64 * 4 * DKMAX = 1024

struct DLevels {
  const void* emb[DMAXL];  // (B, H, W, >= C) NHWC embedding slice of level l, channel 0 of the slice at the pointer
  long psw[DMAXL];         // pixel stride (elements)
  int H[DMAXL], W[DMAXL], a0[DMAXL];
  int nl, A;
};

struct Teacher {
  const void* p;
  long sb, sc, sh, sw;     // element strides of (B, C, h, w): NCHW and NHWC are both just strides
  int h, w;
  int vec;                 // channel stride 1 with aligned base and strides: rows are read with vector loads (else element by element)
};

// ---- four consecutive channels <-> registers ---------------------------------------------------------------------------------
template <typename T> struct Quad;
template <> struct Quad<float> {
  __device__ static __forceinline__ void ld(const float* p, float* f) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    f[0] = __uint_as_float(u.x); f[1] = __uint_as_float(u.y); f[2] = __uint_as_float(u.z); f[3] = __uint_as_float(u.w);
  }
  __device__ static __forceinline__ void st(float* p, const float* f) {
    *reinterpret_cast<uint4*>(p) = make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
  }
};
template <> struct Quad<bf16_t> {
  __device__ static __forceinline__ void ld(const bf16_t* p, float* f) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    f[0] = __uint_as_float(u.x << 16); f[1] = __uint_as_float(u.x & 0xffff0000u);
    f[2] = __uint_as_float(u.y << 16); f[3] = __uint_as_float(u.y & 0xffff0000u);
  }
  __device__ static __forceinline__ void st(bf16_t* p, const float* f) {
    uint2 u;
    u.x = (unsigned)f2bf(f[0]) | ((unsigned)f2bf(f[1]) << 16);
    u.y = (unsigned)f2bf(f[2]) | ((unsigned)f2bf(f[3]) << 16);
    *reinterpret_cast<uint2*>(p) = u;
  }
};

// sum / max over the 64 lanes, the same value in every lane.  The sum uses the DPP row sum and the gfx950 row swaps of common.h
// (a fixed tree: the same bits on every run); the maximum is order-free.
__device__ __forceinline__ float wave_sum(float v) { return lane_xor32_sum(lane_xor16_sum(wave_xor_sum16(v))); }
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
  return v;
}

// ---- count: cnt[b] = number of foreground anchors of image b if it takes part (loss.py:1164), else 0 ----------------------------
__global__ __launch_bounds__(256) void distill_count_kernel(const unsigned char* __restrict__ fg, const float* __restrict__ gt,
                                                            const unsigned char* __restrict__ mixed, int A, int n, int no_mixup,
                                                            int* __restrict__ cnt) {
  __shared__ int sc[256], sv[256];
  const int b = blockIdx.x, t = threadIdx.x;
  int c = 0, v = 0;
  for (int a = t; a < A; a += 256) c += fg[(long)b * A + a] != 0;
  for (int g = t; g < n; g += 256) {  // mask_gt of loss.py:857: the box coordinates sum to more than zero
    const float* r = gt + ((long)b * n + g) * 17;
    v |= (r[1] + r[2] + r[3] + r[4]) > 0.f;
  }
  sc[t] = c;
  sv[t] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) { sc[t] += sc[t + s]; sv[t] |= sv[t + s]; }
    __syncthreads();
  }
  if (t == 0) {
    const bool part = sv[0] != 0 && !(no_mixup && mixed != nullptr && mixed[b] != 0);
    cnt[b] = part ? sc[0] : 0;
  }
}

// ---- index: rows of image b are [sum of cnt[<b], ...) in anchor order; nrows[0] = min(total, cap), nrows[1] = total -----------------
__global__ __launch_bounds__(256) void distill_index_kernel(const unsigned char* __restrict__ fg, const int* __restrict__ cnt, int B,
                                                            int A, int cap, int* __restrict__ idx, int* __restrict__ nrows) {
  __shared__ int sh[256];
  __shared__ int wsum[4];
  const int b = blockIdx.x, t = threadIdx.x;
  int s0 = 0;
  for (int j = t; j < b; j += 256) s0 += cnt[j];
  sh[t] = s0;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) sh[t] += sh[t + s];
    __syncthreads();
  }
  const int base = sh[0], mine = cnt[b];
  if (b == B - 1 && t == 0) {
    const int total = base + mine;
    nrows[0] = total < cap ? total : cap;
    nrows[1] = total;
  }
  if (mine == 0) return;  // (block-uniform) not taking part, or no foreground anchor: no rows
  const int lane = t & 63, wv = t >> 6;
  int run = base;
  for (int a0 = 0; a0 < A; a0 += 256) {
    const int a = a0 + t;
    const bool f = a < A && fg[(long)b * A + a] != 0;
    const unsigned long long m = __ballot(f);
    if (lane == 0) wsum[wv] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { before += k < wv ? wsum[k] : 0; all += wsum[k]; }
    if (f) {
      const int pos = run + before + __popcll(m & ((1ull << lane) - 1ull));
      if (pos < cap) { idx[2 * pos] = b; idx[2 * pos + 1] = a; }
    }
    run += all;
    __syncthreads();
  }
}

// ---- rows ----------------------------------------------------------------------------------------------------------------
// TE: dtype of the embeddings and of the gradient rows (compute dtype); TQ: dtype of the teacher map
template <typename TE, typename TQ>
__global__ __launch_bounds__(256) void distill_rows_kernel(DLevels L, Teacher Q, const float* __restrict__ gt, int n,
                                                           const int* __restrict__ gt_idx, const float* __restrict__ scal,
                                                           const int* __restrict__ cnt, const int* __restrict__ idx,
                                                           const int* __restrict__ nrows, int C, float img_w, float img_h, float T,
                                                           float weight, int crit, TE* __restrict__ rows, float* __restrict__ part) {
  __shared__ float wl[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nr = nrows[0];
  if ((int)blockIdx.x * 4 >= nr) return;  // (block-uniform) the final pass reads ceil(nr / 4) partials only
  const int r = blockIdx.x * 4 + wv;
  float lrow = 0.f;
  if (r < nr) {
    const int b = idx[2 * r], a = idx[2 * r + 1];
    int l = 0;
#pragma unroll
    for (int i = 1; i < DMAXL; ++i) if (i < L.nl && a >= L.a0[i]) l = i;
    const int ra = a - L.a0[l];
    const int hy = ra / L.W[l], hx = ra - hy * L.W[l];
    const TE* e = (const TE*)L.emb[l] + (((long)b * L.H[l] + hy) * L.W[l] + hx) * L.psw[l];
    // teacher pixel of the assigned object (loss.py:1165-1171): round(center_3d / (W, H) * (w, h)), half to even, clamped to the map
    int gi = gt_idx[(long)b * L.A + a];
    gi = gi < 0 ? 0 : (gi > n - 1 ? n - 1 : gi);
    const float* g = gt + ((long)b * n + gi) * 17;
    int tx = (int)rintf(g[9] / img_w * (float)Q.w), ty = (int)rintf(g[10] / img_h * (float)Q.h);
    tx = tx < 0 ? 0 : (tx > Q.w - 1 ? Q.w - 1 : tx);
    ty = ty < 0 ? 0 : (ty > Q.h - 1 ? Q.h - 1 : ty);
    const TQ* q = (const TQ*)Q.p + (long)b * Q.sb + (long)ty * Q.sh + (long)tx * Q.sw;
    const int nch = C >> 2;
    float ev[DKMAX][4], tv[DKMAX][4];
#pragma unroll
    for (int k = 0; k < DKMAX; ++k) {
      const int c = (lane + 64 * k) * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) { ev[k][j] = 0.f; tv[k][j] = 0.f; }
      if (lane + 64 * k < nch) {
        Quad<TE>::ld(e + c, ev[k]);
        if (Q.vec) {
          Quad<TQ>::ld(q + c, tv[k]);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) tv[k][j] = TT<TQ>::ld(q + (long)(c + j) * Q.sc);
        }
      }
    }
    const float nfg = (float)cnt[b], tss = scal[0];
    float gr[DKMAX][4];
    if (crit == 0) {
      // soft (loss.py:1176-1179): sum p_t (log p_t - log_softmax(e / T)) / n_fg * T^2,  p_t = softmax(teacher / T)
      float me = -INFINITY, mt = -INFINITY;
#pragma unroll
      for (int k = 0; k < DKMAX; ++k) {
        const bool on = lane + 64 * k < nch;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          ev[k][j] = ev[k][j] / T;
          tv[k][j] = tv[k][j] / T;
          if (on) { me = fmaxf(me, ev[k][j]); mt = fmaxf(mt, tv[k][j]); }
        }
      }
      me = wave_max(me);
      mt = wave_max(mt);
      float se = 0.f, st = 0.f;
#pragma unroll
      for (int k = 0; k < DKMAX; ++k) {
        if (lane + 64 * k < nch) {
#pragma unroll
          for (int j = 0; j < 4; ++j) { se += expf(ev[k][j] - me); st += expf(tv[k][j] - mt); }
        }
      }
      const float lse_e = me + logf(wave_sum(se)), lse_t = mt + logf(wave_sum(st));
      float acc = 0.f;
      const float gs = T / nfg * weight / tss;
#pragma unroll
      for (int k = 0; k < DKMAX; ++k) {
        const bool on = lane + 64 * k < nch;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float lp = tv[k][j] - lse_t, lq = ev[k][j] - lse_e;
          const float p = expf(lp), qq = expf(lq);
          if (on) acc += p * (lp - lq);
          gr[k][j] = (qq - p) * gs;
        }
      }
      lrow = wave_sum(acc) * (T * T) / nfg;
    } else if (crit == 1) {
      // mse (loss.py:1181, nn.MSELoss): mean over n_fg * C elements
      float acc = 0.f;
      const float den = nfg * (float)C, gs = 2.f / den * weight / tss;
#pragma unroll
      for (int k = 0; k < DKMAX; ++k) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float d = ev[k][j] - tv[k][j];  // (lanes past C hold zeros in both)
          acc += d * d;
          gr[k][j] = d * gs;
        }
      }
      lrow = wave_sum(acc) / den;
    } else {
      // cos (loss.py:1183, nn.CosineEmbeddingLoss, target 1): mean over rows of 1 - e.t / sqrt((|e|^2 + eps)(|t|^2 + eps)); eps is
      // torch's, 1e-12 on the SQUARED norms (aten/native/Loss.cpp cosine_embedding_loss)
      float dot = 0.f, m1 = 0.f, m2 = 0.f;
#pragma unroll
      for (int k = 0; k < DKMAX; ++k) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { dot += ev[k][j] * tv[k][j]; m1 += ev[k][j] * ev[k][j]; m2 += tv[k][j] * tv[k][j]; }
      }
      dot = wave_sum(dot);
      m1 = wave_sum(m1) + 1e-12f;
      m2 = wave_sum(m2) + 1e-12f;
      const float den = sqrtf(m1 * m2), cs = dot / den;
      const float gs = weight / tss / nfg;
#pragma unroll
      for (int k = 0; k < DKMAX; ++k) {
#pragma unroll
        for (int j = 0; j < 4; ++j) gr[k][j] = (cs * ev[k][j] / m1 - tv[k][j] / den) * gs;
      }
      lrow = (1.f - cs) / nfg;
    }
    lrow = lrow * weight / tss;
    TE* o = rows + (long)r * C;
#pragma unroll
    for (int k = 0; k < DKMAX; ++k) {
      if (lane + 64 * k < nch) Quad<TE>::st(o + (lane + 64 * k) * 4, gr[k]);
    }
  }
  if (lane == 0) wl[wv] = lrow;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((wl[0] + wl[1]) + wl[2]) + wl[3];
}

__global__ __launch_bounds__(256) void distill_final_kernel(const float* __restrict__ part, const int* __restrict__ nrows,
                                                            float* __restrict__ loss) {
  __shared__ double sh[256];
  const int t = threadIdx.x, nblk = (nrows[0] + 3) / 4;
  double a = 0.0;
  for (int i = t; i < nblk; i += 256) a += part[i];
  sh[t] = a;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) sh[t] += sh[t + s];
    __syncthreads();
  }
  if (t == 0) loss[0] = (float)sh[0];
}

// ---- scatter: grad[b, pixel of a, 0..C) += scale * row, for the rows whose anchor lies in this level -----------------------------------
// Every (image, anchor) owns at most one row, so the read-modify-write needs no atomic and its result does not depend on any order.
template <typename T>
__global__ __launch_bounds__(256) void distill_scatter_kernel(const T* __restrict__ rows, const int* __restrict__ idx,
                                                              const int* __restrict__ nrows, const float* __restrict__ scale, int C,
                                                              T* __restrict__ grad, long sb, long sh, long sw, int a0, int H, int W) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= nrows[0]) return;
  const int b = idx[2 * r], a = idx[2 * r + 1] - a0;
  if (a < 0 || a >= H * W) return;
  const int hy = a / W, hx = a - hy * W;
  T* gp = grad + (long)b * sb + (long)hy * sh + (long)hx * sw;
  const T* rp = rows + (long)r * C;
  const float s = scale[0];
  for (int c = lane * 4; c < C; c += 256) {
    float g[4], v[4];
    Quad<T>::ld(gp + c, g);
    Quad<T>::ld(rp + c, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = g[j] + v[j] * s;
    Quad<T>::st(gp + c, g);
  }
}

}  // namespace

extern "C" {

int y3d_distill_loss(int dtype, int nl, const void* const* embs, const int64_t* psw, const int* H, const int* W, int B, int C,
                     const void* teacher, int teacher_dtype, int th, int tw, int64_t tsb, int64_t tsc, int64_t tsh, int64_t tsw,
                     const float* gt, int n, const uint8_t* fg_mask, const int* target_gt_idx, const float* scal, const uint8_t* mixed,
                     int img_w, int img_h, float T, float weight, int criterion, int no_mixup, int cap, int* counts, int* idx,
                     void* rows, float* partials, float* loss, void* stream) {
  Y3D_CHECK(dtype == Y3D_BF16 || dtype == Y3D_F32, "distill_loss: bad dtype");
  Y3D_CHECK(teacher_dtype == Y3D_BF16 || teacher_dtype == Y3D_F32, "distill_loss: bad teacher dtype");
  Y3D_CHECK(nl >= 1 && nl <= DMAXL, "distill_loss: 1..%d levels", DMAXL);
  Y3D_CHECK(C >= 8 && C % 8 == 0 && C <= 256 * DKMAX, "distill_loss: C = %d: a multiple of 8 up to %d", C, 256 * DKMAX);
  Y3D_CHECK(B >= 1 && n >= 1 && cap >= 1 && th >= 1 && tw >= 1 && img_w >= 1 && img_h >= 1, "distill_loss: B, n, cap, teacher and image sizes >= 1");
  Y3D_CHECK(criterion >= 0 && criterion <= 2, "distill_loss: criterion %d: 0 soft, 1 mse, 2 cos", criterion);
  Y3D_CHECK(T > 0.f, "distill_loss: temperature must be positive");
  Y3D_CHECK(!no_mixup || mixed != nullptr, "distill_loss: no_mixup needs the per-image `mixed` flags");
  const size_t eb = dtype == Y3D_BF16 ? 8 : 16, qb = teacher_dtype == Y3D_BF16 ? 8 : 16;
  DLevels L;
  int a0 = 0;
  for (int i = 0; i < DMAXL; ++i) {
    if (i < nl) {
      Y3D_CHECK(H[i] >= 1 && W[i] >= 1 && psw[i] >= C && psw[i] % 4 == 0 && (uintptr_t)embs[i] % eb == 0,
                "distill_loss: level %d: the embedding slice must be %zu-byte aligned with a pixel stride that is a multiple of 4 elements", i, eb);
      L.emb[i] = embs[i]; L.psw[i] = psw[i]; L.H[i] = H[i]; L.W[i] = W[i]; L.a0[i] = a0;
      a0 += H[i] * W[i];
    } else {
      L.emb[i] = nullptr; L.psw[i] = 0; L.H[i] = L.W[i] = 1; L.a0[i] = a0;
    }
  }
  L.nl = nl; L.A = a0;
  // vector loads of teacher rows need a unit channel stride and an aligned base / strides (a channel-last map); any other layout,
  // an NCHW map of 1 x 1 pixels included (its channel stride is 1 too), is read element by element through its strides
  const int vec = tsc == 1 && (uintptr_t)teacher % qb == 0 && tsb % 4 == 0 && tsh % 4 == 0 && tsw % 4 == 0;
  Teacher Q{teacher, tsb, tsc, tsh, tsw, th, tw, vec};
  hipStream_t st = (hipStream_t)stream;
  int* cnt = counts;
  int* nrows = counts + B;
  hipLaunchKernelGGL(distill_count_kernel, dim3(B), dim3(256), 0, st, fg_mask, gt, mixed, L.A, n, no_mixup, cnt);
  hipLaunchKernelGGL(distill_index_kernel, dim3(B), dim3(256), 0, st, fg_mask, cnt, B, L.A, cap, idx, nrows);
  const dim3 gr(cdiv(cap, 4));
#define Y3D_DROWS(TE, TQ) hipLaunchKernelGGL((distill_rows_kernel<TE, TQ>), gr, dim3(256), 0, st, L, Q, gt, n, target_gt_idx, scal, cnt, idx, nrows, C, \
                                             (float)img_w, (float)img_h, T, weight, criterion, (TE*)rows, partials)
  if (dtype == Y3D_BF16) { if (teacher_dtype == Y3D_BF16) Y3D_DROWS(bf16_t, bf16_t); else Y3D_DROWS(bf16_t, float); }
  else { if (teacher_dtype == Y3D_BF16) Y3D_DROWS(float, bf16_t); else Y3D_DROWS(float, float); }
#undef Y3D_DROWS
  hipLaunchKernelGGL(distill_final_kernel, dim3(1), dim3(256), 0, st, partials, nrows, loss);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_distill_scatter(int dtype, const void* rows, const int* idx, const int* nrows, const float* scale, int cap, int C, void* grad,
                        int64_t sb, int64_t sh, int64_t sw, int a0, int H, int W, void* stream) {
  Y3D_CHECK(dtype == Y3D_BF16 || dtype == Y3D_F32, "distill_scatter: bad dtype");
  Y3D_CHECK(C >= 8 && C % 8 == 0 && cap >= 1 && H >= 1 && W >= 1 && a0 >= 0, "distill_scatter: C a multiple of 8; cap, H, W >= 1");
  const size_t eb = dtype == Y3D_BF16 ? 8 : 16;
  Y3D_CHECK((uintptr_t)grad % eb == 0 && (uintptr_t)rows % eb == 0 && sb % 4 == 0 && sh % 4 == 0 && sw % 4 == 0,
            "distill_scatter: the gradient slice must be %zu-byte aligned with strides that are multiples of 4 elements", eb);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == Y3D_BF16)
    hipLaunchKernelGGL(distill_scatter_kernel<bf16_t>, dim3(cdiv(cap, 4)), dim3(256), 0, st, (const bf16_t*)rows, idx, nrows, scale, C, (bf16_t*)grad, sb, sh, sw, a0, H, W);
  else
    hipLaunchKernelGGL(distill_scatter_kernel<float>, dim3(cdiv(cap, 4)), dim3(256), 0, st, (const float*)rows, idx, nrows, scale, C, (float*)grad, sb, sh, sw, a0, H, W);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

}  // extern "C"
