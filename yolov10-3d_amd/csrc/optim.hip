// Optimizer side of the training step as three multi-tensor launches:
//   clip_grad_norm_(max_norm) (engine/trainer.py:570, torch.nn.utils.clip_grad_norm_) + SGD with Nesterov momentum and weight decay
//   (trainer.py:571, build_optimizer :734-790; torch.optim.SGD semantics, dampening 0).
// The ~570 parameter tensors are addressed through device tables (pointer, size) and a chunk table (tensor id, offset): one workgroup
// per 16 K-element chunk, 16-byte accesses.  HBM-bound: 16 B read + 8 B written per element for the update, 4 B read for the norm.
#include "common.h"

namespace {

// the chunk of workgroup blockIdx.x: tensor t and its n elements from element off on (tables: mt.chunk_map)
struct Chunk {
  int t;
  long off, n;
};

__device__ __forceinline__ Chunk mt_chunk(const long* __restrict__ sizes, const int* __restrict__ ctensor, const int* __restrict__ coff, int chunk) {
  Chunk ck;
  ck.t = ctensor[blockIdx.x];
  ck.off = (long)coff[blockIdx.x] * chunk;
  ck.n = sizes[ck.t] - ck.off;
  if (ck.n > chunk) ck.n = chunk;
  return ck;
}

__global__ __launch_bounds__(256) void mt_sqnorm_kernel(const long* __restrict__ gptr, const long* __restrict__ sizes, const int* __restrict__ ctensor,
                                                        const int* __restrict__ coff, int chunk, float* __restrict__ partials) {
  __shared__ float sh[256];
  const Chunk ck = mt_chunk(sizes, ctensor, coff, chunk);
  const int t = ck.t;
  const long off = ck.off, n = ck.n;
  const float* g = (const float*)gptr[t] + off;
  float s = 0.f;
  if ((((uintptr_t)g) & 15) == 0) {
    long n4 = n >> 2;
    for (long i = threadIdx.x; i < n4; i += 256) {
      float4 v = ((const float4*)g)[i];
      s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    for (long i = (n4 << 2) + threadIdx.x; i < n; i += 256) s += g[i] * g[i];
  } else {
    for (long i = threadIdx.x; i < n; i += 256) s += g[i] * g[i];
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = sh[0];
}

// out[0] = total L2 norm, out[1] = min(1, max_norm / (norm + 1e-6)), out[2] = 1 if the norm is finite else 0 (the update kernels
// are no-ops for that step: GradScaler.step's skip, engine/trainer.py:569-572), out[3] += out[2] (number of steps applied so far),
// out[4] += 1 - out[2] (number of steps skipped)
__global__ __launch_bounds__(256) void mt_clip_kernel(const float* __restrict__ partials, int n, float max_norm, float* __restrict__ out) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)partials[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float norm = (float)sqrt(sh[0]);
    float c = max_norm / (norm + 1e-6f);
    const bool ok = isfinite(norm);
    out[0] = norm;
    out[1] = c < 1.f ? c : 1.f;
    out[2] = ok ? 1.f : 0.f;
    out[3] += ok ? 1.f : 0.f;
    out[4] += ok ? 0.f : 1.f;
  }
}

// one element of torch.optim.SGD (dampening 0), for mt_sgd_kernel and mt_sgd_tab_kernel
__device__ __forceinline__ void upd_sgd(float& p, const float g, float& b, float c, float l, float w, float momentum, int nesterov, int first) {
  const float pv = p;
  float gv = g * c;
  if (w != 0.f) gv += w * pv;
  const float bv = first ? gv : momentum * b + gv;
  b = bv;
  const float step = nesterov ? gv + momentum * bv : bv;
  p = pv - l * step;
}

__global__ __launch_bounds__(256) void mt_sgd_kernel(const long* __restrict__ pptr, const long* __restrict__ gptr, const long* __restrict__ bptr,
                                                     const long* __restrict__ sizes, const float* __restrict__ lr, const float* __restrict__ wd,
                                                     const int* __restrict__ ctensor, const int* __restrict__ coff, int chunk, float momentum,
                                                     int nesterov, int first, const float* __restrict__ clip) {
  const Chunk ck = mt_chunk(sizes, ctensor, coff, chunk);
  const int t = ck.t;
  const long off = ck.off, n = ck.n;
  float* p = (float*)pptr[t] + off;
  const float* g = (const float*)gptr[t] + off;
  float* b = (float*)bptr[t] + off;
  if (clip && clip[2] == 0.f) return;  // non-finite gradient norm: this step is skipped on every rank (the norm is that of the reduced buffer)
  const float c = clip ? clip[1] : 1.f, l = lr[t], w = wd[t];
  for (long i = threadIdx.x; i < n; i += 256) upd_sgd(p[i], g[i], b[i], c, l, w, momentum, nesterov, first);
}

// dst_t[i] = src_t[i] * scale for every tensor t of the table: gathers the step's gradient tensors into the flat all-reduce buffer
__global__ __launch_bounds__(256) void mt_copy_kernel(const long* __restrict__ sptr, const long* __restrict__ dptr, const long* __restrict__ sizes,
                                                      const int* __restrict__ ctensor, const int* __restrict__ coff, int chunk, float scale) {
  const Chunk ck = mt_chunk(sizes, ctensor, coff, chunk);
  const int t = ck.t;
  const long off = ck.off, n = ck.n;
  const float* s = (const float*)sptr[t] + off;
  float* d = (float*)dptr[t] + off;
  if (((((uintptr_t)s) | ((uintptr_t)d)) & 15) == 0) {
    const long n4 = n >> 2;
    for (long i = threadIdx.x; i < n4; i += 256) {
      float4 v = ((const float4*)s)[i];
      ((float4*)d)[i] = make_float4(v.x * scale, v.y * scale, v.z * scale, v.w * scale);
    }
    for (long i = (n4 << 2) + threadIdx.x; i < n; i += 256) d[i] = s[i] * scale;
  } else {
    for (long i = threadIdx.x; i < n; i += 256) d[i] = s[i] * scale;
  }
}


// torch.optim.AdamW (amsgrad off, maximize off), one parameter chunk per workgroup.  bc1 = 1 - beta1^step, bc2s = sqrt(1 - beta2^step).
__global__ __launch_bounds__(256) void mt_adamw_kernel(const long* __restrict__ pptr, const long* __restrict__ gptr, const long* __restrict__ mptr,
                                                       const long* __restrict__ vptr, const long* __restrict__ sizes, const float* __restrict__ lr,
                                                       const float* __restrict__ wd, const int* __restrict__ ctensor, const int* __restrict__ coff,
                                                       int chunk, float beta1, float beta2, float eps, float bc1, float bc2s,
                                                       const float* __restrict__ clip) {
  const Chunk ck = mt_chunk(sizes, ctensor, coff, chunk);
  const int t = ck.t;
  const long off = ck.off, n = ck.n;
  float* p = (float*)pptr[t] + off;
  const float* g = (const float*)gptr[t] + off;
  float* m = (float*)mptr[t] + off;
  float* v = (float*)vptr[t] + off;
  if (clip) {
    if (clip[2] == 0.f) return;  // skipped step (non-finite gradient norm): state and step count stay
    // the step count of the bias corrections is the number of APPLIED steps, which only the device knows
    const double tstep = (double)clip[3];
    bc1 = (float)(1.0 - pow((double)beta1, tstep));
    bc2s = (float)sqrt(1.0 - pow((double)beta2, tstep));
  }
  const float c = clip ? clip[1] : 1.f, l = lr[t], w = wd[t];
  const float step_size = l / bc1, decay = 1.f - l * w, w1 = 1.f - beta1, w2 = 1.f - beta2;
  for (long i = threadIdx.x; i < n; i += 256) {
    const float gv = g[i] * c;
    const float pv = p[i] * decay;
    const float mv = m[i] + w1 * (gv - m[i]);  // exp_avg.lerp_(grad, 1 - beta1)
    const float vv = v[i] * beta2 + w2 * gv * gv;
    m[i] = mv;
    v[i] = vv;
    p[i] = pv - step_size * (mv / (sqrtf(vv) / bc2s + eps));
  }
}

// ---- the reference's remaining optimizers (engine/trainer.py:776-781: Adam, Adamax, NAdam, RAdam, RMSProp) --------------------------------
// Everything that depends only on the number of APPLIED steps is computed once per step by mt_step_scalars_kernel (double, rounded once
// to float) into a Y3D_STEP_SCALARS-float array; the update kernels read it.  Index names: include/y3d.h.
enum { S_BC1 = 0, S_BC2, S_BC1_SQRT, S_BC2_SQRT, S_MU, S_MU_NEXT, S_MU_PROD, S_MU_PROD_NEXT, S_RHO, S_RECT_ON, S_RECT, S_T, S_NADAM_G, S_NADAM_M };
enum { K_ADAM = 0, K_ADAMAX = 1, K_NADAM = 2, K_RADAM = 3, K_RMSPROP = 4 };

// clip: mt_clip_kernel's array.  A skipped step (clip[2] == 0) leaves every scalar, mu_product included, as it is.
__global__ __launch_bounds__(64) void mt_step_scalars_kernel(const float* __restrict__ clip, float beta1, float beta2, double momentum_decay,
                                                             float* __restrict__ scal) {
  if (threadIdx.x != 0 || clip[2] == 0.f) return;
  const double t = (double)clip[3], b1 = (double)beta1, b2 = (double)beta2;
  const double p2 = pow(b2, t);
  const double bc1 = 1.0 - pow(b1, t), bc2 = 1.0 - p2;
  scal[S_BC1] = (float)bc1;
  scal[S_BC2] = (float)bc2;
  scal[S_BC1_SQRT] = (float)sqrt(bc1);
  scal[S_BC2_SQRT] = (float)sqrt(bc2);
  // torch.optim.NAdam: mu_t, mu_{t+1}, and mu_product *= mu_t (fp32 state; 1 before the first applied step)
  const double mu = b1 * (1.0 - 0.5 * pow(0.96, t * momentum_decay));
  const double mu_next = b1 * (1.0 - 0.5 * pow(0.96, (t + 1.0) * momentum_decay));
  const float mp = (float)((double)(t == 1.0 ? 1.f : scal[S_MU_PROD]) * mu);
  const double mp_next = (double)mp * mu_next;
  scal[S_MU] = (float)mu;
  scal[S_MU_NEXT] = (float)mu_next;
  scal[S_MU_PROD] = mp;
  scal[S_MU_PROD_NEXT] = (float)mp_next;
  scal[S_NADAM_G] = (float)((1.0 - mu) / (1.0 - (double)mp));
  scal[S_NADAM_M] = (float)(mu_next / (1.0 - mp_next));
  // torch.optim.RAdam: length of the approximated SMA, the rho_t > 5 decision (taken in double) and the rectification factor
  const double rho_inf = 2.0 / (1.0 - b2) - 1.0;
  const double rho = rho_inf - 2.0 * t * p2 / bc2;
  const bool on = rho > 5.0;
  scal[S_RHO] = (float)rho;
  scal[S_RECT_ON] = on ? 1.f : 0.f;
  scal[S_RECT] = on ? (float)sqrt((rho - 4.0) * (rho - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho)) : 0.f;
  scal[S_T] = (float)t;
}

// per-workgroup constants of one tensor's update; k0..k2 and arm by kind (mt_update_kernel)
struct UpdCoef {
  float c, l, w, b2, w1, w2, eps, k0, k1, k2;
  int arm;
};

// one element, torch's single-tensor arithmetic (foreach=False, not capturable).  a, b: the two state buffers
//   Adam / NAdam / RAdam: exp_avg, exp_avg_sq;  Adamax: exp_avg, exp_inf;  RMSprop: square_avg, momentum_buffer
template <int KIND>
__device__ __forceinline__ void upd(float& p, const float g, float& a, float& b, const UpdCoef& k) {
  const float pv = p;
  float gv = g * k.c;
  if (k.w != 0.f) gv += k.w * pv;  // coupled L2 decay: grad.add(param, alpha=weight_decay)
  if (KIND == K_RMSPROP) {
    const float sq = a * k.b2 + k.w2 * gv * gv;  // square_avg.mul_(alpha).addcmul_(grad, grad, value=1 - alpha)
    a = sq;
    const float q = gv / (sqrtf(sq) + k.eps);
    if (k.arm) {  // momentum > 0
      const float bv = b * k.k0 + q;
      b = bv;
      p = pv - k.l * bv;
    } else {
      p = pv - k.l * q;
    }
    return;
  }
  const float mv = a + k.w1 * (gv - a);  // exp_avg.lerp_(grad, 1 - beta1)
  a = mv;
  if (KIND == K_ADAMAX) {
    const float d = b * k.b2, e = fabsf(gv) + k.eps;
    const float un = d > e ? d : e;  // exp_inf = max(beta2 * exp_inf, |grad| + eps)
    b = un;
    p = pv - k.k0 * (mv / un);  // k0 = lr / (1 - beta1^t)
    return;
  }
  const float vv = b * k.b2 + k.w2 * gv * gv;
  b = vv;
  if (KIND == K_ADAM) {  // k0 = lr / (1 - beta1^t), k1 = sqrt(1 - beta2^t)
    p = pv - k.k0 * (mv / (sqrtf(vv) / k.k1 + k.eps));
  } else if (KIND == K_NADAM) {  // k0 = lr (1 - mu_t) / (1 - mu_product), k1 = lr mu_{t+1} / (1 - mu_product mu_{t+1}), k2 = 1 - beta2^t
    const float denom = sqrtf(vv / k.k2) + k.eps;
    const float p1 = pv - k.k0 * (gv / denom);
    p = p1 - k.k1 * (mv / denom);
  } else {  // K_RADAM: k0 = 1 - beta1^t, k1 = sqrt(1 - beta2^t), k2 = rectification factor, arm = rho_t > 5
    const float bce = mv / k.k0;
    if (k.arm) p = pv - ((bce * k.l) * (k.k1 / (sqrtf(vv) + k.eps))) * k.k2;
    else p = pv - bce * k.l;
  }
}

// One parameter chunk per workgroup, chunk tables and skip rule of mt_sgd / mt_adamw.  16-byte accesses when the four pointers allow.
// mom: per-tensor momentum table (RMSprop only); scal: mt_step_scalars_kernel's array (not read by RMSprop).
template <int KIND>
__global__ __launch_bounds__(256) void mt_update_kernel(const long* __restrict__ pptr, const long* __restrict__ gptr, const long* __restrict__ aptr,
                                                        const long* __restrict__ bptr, const long* __restrict__ sizes, const float* __restrict__ lr,
                                                        const float* __restrict__ wd, const float* __restrict__ mom, const int* __restrict__ ctensor,
                                                        const int* __restrict__ coff, int chunk, float beta1, float beta2, float eps,
                                                        const float* __restrict__ scal, const float* __restrict__ clip) {
  const Chunk ck = mt_chunk(sizes, ctensor, coff, chunk);
  const int t = ck.t;
  const long off = ck.off, n = ck.n;
  float* p = (float*)pptr[t] + off;
  const float* g = (const float*)gptr[t] + off;
  float* a = (float*)aptr[t] + off;
  float* b = (float*)bptr[t] + off;
  if (clip && clip[2] == 0.f) return;  // skipped step (non-finite gradient norm): parameters and state stay
  UpdCoef k;
  k.c = clip ? clip[1] : 1.f;
  k.l = lr[t];
  k.w = wd[t];
  k.b2 = beta2;
  k.w1 = 1.f - beta1;
  k.w2 = 1.f - beta2;
  k.eps = eps;
  k.k0 = k.k1 = k.k2 = 0.f;
  k.arm = 0;
  if (KIND == K_ADAM) {
    k.k0 = k.l / scal[S_BC1];
    k.k1 = scal[S_BC2_SQRT];
  } else if (KIND == K_ADAMAX) {
    k.k0 = k.l / scal[S_BC1];
  } else if (KIND == K_NADAM) {
    k.k0 = k.l * scal[S_NADAM_G];
    k.k1 = k.l * scal[S_NADAM_M];
    k.k2 = scal[S_BC2];
  } else if (KIND == K_RADAM) {
    k.k0 = scal[S_BC1];
    k.k1 = scal[S_BC2_SQRT];
    k.k2 = scal[S_RECT];
    k.arm = scal[S_RECT_ON] != 0.f;
  } else {
    k.k0 = mom[t];
    k.arm = k.k0 > 0.f;
  }
  if (((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0) {
    const long n4 = n >> 2;
    for (long i = threadIdx.x; i < n4; i += 256) {
      float4 P = ((float4*)p)[i], A = ((float4*)a)[i], B = ((float4*)b)[i];
      const float4 G = ((const float4*)g)[i];
      upd<KIND>(P.x, G.x, A.x, B.x, k);
      upd<KIND>(P.y, G.y, A.y, B.y, k);
      upd<KIND>(P.z, G.z, A.z, B.z, k);
      upd<KIND>(P.w, G.w, A.w, B.w, k);
      ((float4*)a)[i] = A;
      ((float4*)b)[i] = B;
      ((float4*)p)[i] = P;
    }
    for (long i = (n4 << 2) + threadIdx.x; i < n; i += 256) upd<KIND>(p[i], g[i], a[i], b[i], k);
  } else {
    for (long i = threadIdx.x; i < n; i += 256) upd<KIND>(p[i], g[i], a[i], b[i], k);
  }
}

// mt_sgd_kernel with the momentum read from a per-tensor device table next to lr / wd: a captured step follows a momentum schedule
// (warm-up, engine/trainer.py:392-393) through in-place writes of the table
__global__ __launch_bounds__(256) void mt_sgd_tab_kernel(const long* __restrict__ pptr, const long* __restrict__ gptr, const long* __restrict__ bptr,
                                                         const long* __restrict__ sizes, const float* __restrict__ lr, const float* __restrict__ wd,
                                                         const float* __restrict__ mom, const int* __restrict__ ctensor, const int* __restrict__ coff,
                                                         int chunk, int nesterov, int first, const float* __restrict__ clip) {
  const Chunk ck = mt_chunk(sizes, ctensor, coff, chunk);
  const int t = ck.t;
  const long off = ck.off, n = ck.n;
  float* p = (float*)pptr[t] + off;
  const float* g = (const float*)gptr[t] + off;
  float* b = (float*)bptr[t] + off;
  if (clip && clip[2] == 0.f) return;
  const float c = clip ? clip[1] : 1.f, l = lr[t], w = wd[t], m = mom[t];
  if (((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)b)) & 15) == 0) {
    const long n4 = n >> 2;
    for (long i = threadIdx.x; i < n4; i += 256) {
      float4 P = ((float4*)p)[i], B = ((float4*)b)[i];
      const float4 G = ((const float4*)g)[i];
      upd_sgd(P.x, G.x, B.x, c, l, w, m, nesterov, first);
      upd_sgd(P.y, G.y, B.y, c, l, w, m, nesterov, first);
      upd_sgd(P.z, G.z, B.z, c, l, w, m, nesterov, first);
      upd_sgd(P.w, G.w, B.w, c, l, w, m, nesterov, first);
      ((float4*)b)[i] = B;
      ((float4*)p)[i] = P;
    }
    for (long i = (n4 << 2) + threadIdx.x; i < n; i += 256) upd_sgd(p[i], g[i], b[i], c, l, w, m, nesterov, first);
  } else {
    for (long i = threadIdx.x; i < n; i += 256) upd_sgd(p[i], g[i], b[i], c, l, w, m, nesterov, first);
  }
}

// ModelEMA.update (utils/torch_utils.py:431-443): e = e * d + (1 - d) * m, applied reps[t] times to tensor t (an EMA tensor that the
// reference's state_dict lists under several keys -- the aliased one-to-one head branches -- is updated once per key)
__global__ __launch_bounds__(256) void mt_ema_kernel(const long* __restrict__ eptr, const long* __restrict__ mptr, const long* __restrict__ sizes,
                                                     const int* __restrict__ reps, const int* __restrict__ ctensor, const int* __restrict__ coff,
                                                     int chunk, float d, float omd, const float* __restrict__ guard) {
  if (guard && guard[2] == 0.f) return;  // the optimizer step this update follows was skipped: the model did not move
  const Chunk ck = mt_chunk(sizes, ctensor, coff, chunk);
  const int t = ck.t;
  const long off = ck.off, n = ck.n;
  float* e = (float*)eptr[t] + off;
  const float* m = (const float*)mptr[t] + off;
  const int r = reps[t];
  for (long i = threadIdx.x; i < n; i += 256) {
    float ev = e[i];
    const float mv = omd * m[i];
    for (int k = 0; k < r; ++k) ev = ev * d + mv;
    e[i] = ev;
  }
}

// acc_t[i] += grad_t[i] for every tensor t of the table: one micro-batch's gradients added into the accumulation arena
// (optim.GradAccumulator; reference: autograd's AccumulateGrad over the `accumulate` backward passes of one optimizer step,
// engine/trainer.py:384-386, 411-413).  Tables and chunking of mt_copy_kernel; 8 B read + 4 B written per element.
__global__ __launch_bounds__(256) void mt_grad_acc_kernel(const long* __restrict__ aptr, const long* __restrict__ gptr, const long* __restrict__ sizes,
                                                          const int* __restrict__ ctensor, const int* __restrict__ coff, int chunk) {
  const Chunk ck = mt_chunk(sizes, ctensor, coff, chunk);
  const int t = ck.t;
  const long off = ck.off, n = ck.n;
  float* a = (float*)aptr[t] + off;
  const float* g = (const float*)gptr[t] + off;
  if (((((uintptr_t)a) | ((uintptr_t)g)) & 15) == 0) {
    const long n4 = n >> 2;
    for (long i = threadIdx.x; i < n4; i += 256) {
      float4 A = ((float4*)a)[i];
      const float4 G = ((const float4*)g)[i];
      A.x += G.x;
      A.y += G.y;
      A.z += G.z;
      A.w += G.w;
      ((float4*)a)[i] = A;
    }
    for (long i = (n4 << 2) + threadIdx.x; i < n; i += 256) a[i] += g[i];
  } else {
    for (long i = threadIdx.x; i < n; i += 256) a[i] += g[i];
  }
}

}  // namespace

extern "C" {

int y3d_mt_grad_acc(const int64_t* acc_ptrs, const int64_t* grad_ptrs, const int64_t* sizes, const int* chunk_tensor, const int* chunk_off,
                    int nchunks, int chunk, void* stream) {
  Y3D_CHECK(nchunks >= 1 && chunk >= 256, "mt_grad_acc: empty chunk table");
  hipLaunchKernelGGL(mt_grad_acc_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, (const long*)acc_ptrs, (const long*)grad_ptrs,
                     (const long*)sizes, chunk_tensor, chunk_off, chunk);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_mt_copy(const int64_t* src_ptrs, const int64_t* dst_ptrs, const int64_t* sizes, const int* chunk_tensor, const int* chunk_off,
                int nchunks, int chunk, float scale, void* stream) {
  Y3D_CHECK(nchunks >= 1 && chunk >= 256, "mt_copy: empty chunk table");
  hipLaunchKernelGGL(mt_copy_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, (const long*)src_ptrs, (const long*)dst_ptrs,
                     (const long*)sizes, chunk_tensor, chunk_off, chunk, scale);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}


int y3d_mt_sqnorm(const int64_t* grad_ptrs, const int64_t* sizes, const int* chunk_tensor, const int* chunk_off, int nchunks, int chunk,
                  float* partials, void* stream) {
  Y3D_CHECK(nchunks >= 1 && chunk >= 256, "mt_sqnorm: empty chunk table");
  hipLaunchKernelGGL(mt_sqnorm_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, (const long*)grad_ptrs, (const long*)sizes, chunk_tensor,
                     chunk_off, chunk, partials);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_mt_clip_coef(const float* partials, int nchunks, float max_norm, float* out_norm_clip, void* stream) {
  hipLaunchKernelGGL(mt_clip_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, nchunks, max_norm, out_norm_clip);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_mt_sgd(const int64_t* param_ptrs, const int64_t* grad_ptrs, const int64_t* buf_ptrs, const int64_t* sizes, const float* lr,
               const float* wd, const int* chunk_tensor, const int* chunk_off, int nchunks, int chunk, float momentum, int nesterov,
               int first_step, const float* norm_clip, void* stream) {
  Y3D_CHECK(nchunks >= 1 && chunk >= 256, "mt_sgd: empty chunk table");
  hipLaunchKernelGGL(mt_sgd_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, (const long*)param_ptrs, (const long*)grad_ptrs,
                     (const long*)buf_ptrs, (const long*)sizes, lr, wd, chunk_tensor, chunk_off, chunk, momentum, nesterov, first_step, norm_clip);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_mt_adamw(const int64_t* param_ptrs, const int64_t* grad_ptrs, const int64_t* m_ptrs, const int64_t* v_ptrs, const int64_t* sizes,
                 const float* lr, const float* wd, const int* chunk_tensor, const int* chunk_off, int nchunks, int chunk, float beta1, float beta2,
                 float eps, float bias_corr1, float bias_corr2_sqrt, const float* norm_clip, void* stream) {
  Y3D_CHECK(nchunks >= 1 && chunk >= 256, "mt_adamw: empty chunk table");
  Y3D_CHECK(bias_corr1 > 0.f && bias_corr2_sqrt > 0.f, "mt_adamw: bias corrections must be positive (step >= 1)");
  hipLaunchKernelGGL(mt_adamw_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, (const long*)param_ptrs, (const long*)grad_ptrs,
                     (const long*)m_ptrs, (const long*)v_ptrs, (const long*)sizes, lr, wd, chunk_tensor, chunk_off, chunk, beta1, beta2, eps,
                     bias_corr1, bias_corr2_sqrt, norm_clip);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_mt_step_scalars(const float* norm_clip, float beta1, float beta2, double momentum_decay, float* step_scalars, void* stream) {
  Y3D_CHECK(norm_clip && step_scalars, "mt_step_scalars: null array");
  Y3D_CHECK(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "mt_step_scalars: betas must lie in [0, 1)");
  hipLaunchKernelGGL(mt_step_scalars_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, norm_clip, beta1, beta2, momentum_decay, step_scalars);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_mt_update(int kind, const int64_t* param_ptrs, const int64_t* grad_ptrs, const int64_t* s0_ptrs, const int64_t* s1_ptrs,
                  const int64_t* sizes, const float* lr, const float* wd, const float* momentum, const int* chunk_tensor, const int* chunk_off,
                  int nchunks, int chunk, float beta1, float beta2, float eps, const float* step_scalars, const float* norm_clip, void* stream) {
  Y3D_CHECK(nchunks >= 1 && chunk >= 256, "mt_update: empty chunk table");
  Y3D_CHECK(kind >= K_ADAM && kind <= K_RMSPROP, "mt_update: kind must be one of Y3D_OPT_ADAM .. Y3D_OPT_RMSPROP");
  Y3D_CHECK(kind == K_RMSPROP ? momentum != nullptr : step_scalars != nullptr,
            "mt_update: RMSprop needs the momentum table, the Adam family the step scalars");
#define Y3D_UPD(K)                                                                                                                             \
  hipLaunchKernelGGL(mt_update_kernel<K>, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, (const long*)param_ptrs, (const long*)grad_ptrs,   \
                     (const long*)s0_ptrs, (const long*)s1_ptrs, (const long*)sizes, lr, wd, momentum, chunk_tensor, chunk_off, chunk, beta1,  \
                     beta2, eps, step_scalars, norm_clip)
  switch (kind) {
    case K_ADAM: Y3D_UPD(K_ADAM); break;
    case K_ADAMAX: Y3D_UPD(K_ADAMAX); break;
    case K_NADAM: Y3D_UPD(K_NADAM); break;
    case K_RADAM: Y3D_UPD(K_RADAM); break;
    default: Y3D_UPD(K_RMSPROP); break;
  }
#undef Y3D_UPD
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_mt_sgd_tab(const int64_t* param_ptrs, const int64_t* grad_ptrs, const int64_t* buf_ptrs, const int64_t* sizes, const float* lr,
                   const float* wd, const float* momentum, const int* chunk_tensor, const int* chunk_off, int nchunks, int chunk, int nesterov,
                   int first_step, const float* norm_clip, void* stream) {
  Y3D_CHECK(nchunks >= 1 && chunk >= 256, "mt_sgd_tab: empty chunk table");
  Y3D_CHECK(momentum, "mt_sgd_tab: null momentum table");
  hipLaunchKernelGGL(mt_sgd_tab_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, (const long*)param_ptrs, (const long*)grad_ptrs,
                     (const long*)buf_ptrs, (const long*)sizes, lr, wd, momentum, chunk_tensor, chunk_off, chunk, nesterov, first_step, norm_clip);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_mt_ema(const int64_t* ema_ptrs, const int64_t* model_ptrs, const int64_t* sizes, const int* reps, const int* chunk_tensor,
               const int* chunk_off, int nchunks, int chunk, float decay, float one_minus_decay, const float* guard, void* stream) {
  Y3D_CHECK(nchunks >= 1 && chunk >= 256, "mt_ema: empty chunk table");
  hipLaunchKernelGGL(mt_ema_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, (const long*)ema_ptrs, (const long*)model_ptrs,
                     (const long*)sizes, reps, chunk_tensor, chunk_off, chunk, decay, one_minus_decay, guard);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

}  // extern "C"
