// Bilinear resize of an NHWC map to any output size, forward and adjoint (F.interpolate(mode="bilinear", align_corners=False) and its
// autograd backward; nn/modules/head.py:1021: the depth predictor brings P5 to P4's size - 13 -> 25 rows at H = 400 is no exact 2x).
//
// ATen's rule, in float32 as ATen computes it: scale = (float)in / out, src = max(scale * (dst + 0.5) - 0.5, 0), i0 = min((int)src, in - 1),
// i1 = i0 + (i0 < in - 1), l1 = clamp(src - i0, 0, 1), l0 = 1 - l1;  y[oy][ox] = h0 (w0 x[y0][x0] + w1 x[y0][x1]) + h1 (w0 x[y1][x0] + w1 x[y1][x1]).
//
// One thread owns one 16-byte channel chunk of one pixel: of the OUTPUT in the forward, of the INPUT in the adjoint.  The adjoint is a
// gather: an input pixel (iy, ix) walks the output rows and columns whose i0 or i1 can be iy / ix (a window around (iy + 0.5) / scale,
// widened by one on both sides and tested with the forward's own index function) in ascending order and adds w_y w_x dy: no atomics,
// the same bits on every run.  The forward's arithmetic is fp32, the result rounded once to the map's dtype.  The adjoint sums in
// double (an input pixel of a 2x map collects up to 16 terms whose weights add up to 4: the sum outgrows its terms, and fp32 partial sums
// would cost several ulps of it) and rounds once.
#include "common.h"

namespace {

struct BilIdx { int i0, i1; float l0, l1; };

__device__ __forceinline__ BilIdx bil_index(int dst, float scale, int in) {
  float s = scale * ((float)dst + 0.5f) - 0.5f;
  if (s < 0.f) s = 0.f;
  BilIdx r;
  r.i0 = (int)s;
  if (r.i0 > in - 1) r.i0 = in - 1;
  r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
  float l = s - (float)r.i0;
  r.l1 = l < 0.f ? 0.f : (l > 1.f ? 1.f : l);
  r.l0 = 1.f - r.l1;
  return r;
}

// the weight output index `dst` gives input index `i` (0 when it reads neither as i0 nor as i1; both at the upper clamp)
__device__ __forceinline__ float bil_weight(int dst, float scale, int in, int i) {
  const BilIdx r = bil_index(dst, scale, in);
  return (r.i0 == i ? r.l0 : 0.f) + (r.i1 == i ? r.l1 : 0.f);
}

// first / last output index that can read input index i, clamped to [0, out - 1]
__device__ __forceinline__ void bil_window(int i, float scale, int out, int& lo, int& hi) {
  lo = (int)floorf(((float)i - 0.5f) / scale - 0.5f) - 1;
  hi = (int)ceilf(((float)i + 1.5f) / scale - 0.5f) + 1;
  if (lo < 0) lo = 0;
  if (hi > out - 1) hi = out - 1;
}

template <typename T>
__global__ __launch_bounds__(256) void resize_fwd_kernel(const T* __restrict__ x, long sb, long sh, long sw, T* __restrict__ y, long ysw, int B,
                                                         int H, int W, int Ho, int Wo, int C) {
  constexpr int CE = TT<T>::CE;
  const int cpp = C / CE;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x, total = (long)B * Ho * Wo * cpp;
  if (idx >= total) return;
  const int k = (int)(idx % cpp);
  const long pix = idx / cpp;
  const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), b = (int)(pix / ((long)Wo * Ho));
  const BilIdx ry = bil_index(oy, (float)H / (float)Ho, H), rx = bil_index(ox, (float)W / (float)Wo, W);
  const T* xb = x + (long)b * sb + k * CE;
  float a[CE], bq[CE], c[CE], d[CE], o[CE];
  Chunk<T>::unpack(*reinterpret_cast<const uint4*>(xb + ry.i0 * sh + rx.i0 * sw), a);
  Chunk<T>::unpack(*reinterpret_cast<const uint4*>(xb + ry.i0 * sh + rx.i1 * sw), bq);
  Chunk<T>::unpack(*reinterpret_cast<const uint4*>(xb + ry.i1 * sh + rx.i0 * sw), c);
  Chunk<T>::unpack(*reinterpret_cast<const uint4*>(xb + ry.i1 * sh + rx.i1 * sw), d);
#pragma unroll
  for (int e = 0; e < CE; ++e) o[e] = ry.l0 * (rx.l0 * a[e] + rx.l1 * bq[e]) + ry.l1 * (rx.l0 * c[e] + rx.l1 * d[e]);
  *reinterpret_cast<uint4*>(y + pix * ysw + k * CE) = Chunk<T>::pack(o);
}

template <typename T>
__global__ __launch_bounds__(256) void resize_bwd_kernel(const T* __restrict__ dy, long dsw, T* __restrict__ dx, long xsw, int B, int H, int W,
                                                         int Ho, int Wo, int C) {
  constexpr int CE = TT<T>::CE;
  const int cpp = C / CE;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x, total = (long)B * H * W * cpp;
  if (idx >= total) return;
  const int k = (int)(idx % cpp);
  const long pix = idx / cpp;
  const int ix = (int)(pix % W), iy = (int)((pix / W) % H), b = (int)(pix / ((long)W * H));
  const float scy = (float)H / (float)Ho, scx = (float)W / (float)Wo;
  int ylo, yhi, xlo, xhi;
  bil_window(iy, scy, Ho, ylo, yhi);
  bil_window(ix, scx, Wo, xlo, xhi);
  double acc[CE];
#pragma unroll
  for (int e = 0; e < CE; ++e) acc[e] = 0.0;
  const T* db = dy + (long)b * Ho * Wo * dsw + k * CE;
  for (int oy = ylo; oy <= yhi; ++oy) {
    const float wy = bil_weight(oy, scy, H, iy);
    if (wy == 0.f) continue;
    for (int ox = xlo; ox <= xhi; ++ox) {
      const float wx = bil_weight(ox, scx, W, ix);
      if (wx == 0.f) continue;
      float g[CE];
      Chunk<T>::unpack(*reinterpret_cast<const uint4*>(db + ((long)oy * Wo + ox) * dsw), g);
      const double wgt = (double)wy * (double)wx;
#pragma unroll
      for (int e = 0; e < CE; ++e) acc[e] += wgt * (double)g[e];
    }
  }
  float o[CE];
#pragma unroll
  for (int e = 0; e < CE; ++e) o[e] = (float)acc[e];
  *reinterpret_cast<uint4*>(dx + pix * xsw + k * CE) = Chunk<T>::pack(o);
}

int resize_check(const char* who, int dtype, const void* a, const void* b, int B, int H, int W, int Ho, int Wo, int C, int64_t s0, int64_t s1) {
  Y3D_CHECK(dtype == Y3D_BF16 || dtype == Y3D_F32, "%s: bad dtype", who);
  const int ce = dtype == Y3D_BF16 ? 8 : 4;
  Y3D_CHECK(B >= 1 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1, "%s: empty shape", who);
  Y3D_CHECK(C >= 8 && C % 8 == 0, "%s: C = %d must be a multiple of 8", who, C);
  Y3D_CHECK(a != nullptr && b != nullptr && (uintptr_t)a % 16 == 0 && (uintptr_t)b % 16 == 0, "%s: 16-byte aligned, non-null maps", who);
  Y3D_CHECK(s0 >= C && s0 % ce == 0 && s1 >= C && s1 % ce == 0, "%s: pixel strides >= C in whole 16-byte chunks", who);
  Y3D_CHECK((long)B * (H > Ho ? H : Ho) * (W > Wo ? W : Wo) * (C / ce) < (1L << 31) * 256, "%s: map too large", who);
  return Y3D_OK;
}

}  // namespace

extern "C" {

int y3d_resize_bilinear_fwd(int dtype, const void* x, int64_t xsb, int64_t xsh, int64_t xsw, void* y, int64_t ysw, int B, int H, int W, int Ho,
                            int Wo, int C, void* stream) {
  if (int rc = resize_check("resize_bilinear_fwd", dtype, x, y, B, H, W, Ho, Wo, C, xsw, ysw)) return rc;
  const int ce = dtype == Y3D_BF16 ? 8 : 4;
  Y3D_CHECK(xsb % ce == 0 && xsh % ce == 0 && xsb >= 0 && xsh >= 0, "resize_bilinear_fwd: x strides in whole 16-byte chunks");
  const long total = (long)B * Ho * Wo * (C / ce);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == Y3D_BF16)
    hipLaunchKernelGGL(resize_fwd_kernel<bf16_t>, dim3(cdiv(total, 256)), dim3(256), 0, st, (const bf16_t*)x, (long)xsb, (long)xsh, (long)xsw,
                       (bf16_t*)y, (long)ysw, B, H, W, Ho, Wo, C);
  else
    hipLaunchKernelGGL(resize_fwd_kernel<float>, dim3(cdiv(total, 256)), dim3(256), 0, st, (const float*)x, (long)xsb, (long)xsh, (long)xsw,
                       (float*)y, (long)ysw, B, H, W, Ho, Wo, C);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

int y3d_resize_bilinear_bwd(int dtype, const void* dy, int64_t dsw, void* dx, int64_t xsw, int B, int H, int W, int Ho, int Wo, int C,
                            void* stream) {
  if (int rc = resize_check("resize_bilinear_bwd", dtype, dy, dx, B, H, W, Ho, Wo, C, dsw, xsw)) return rc;
  const int ce = dtype == Y3D_BF16 ? 8 : 4;
  const long total = (long)B * H * W * (C / ce);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == Y3D_BF16)
    hipLaunchKernelGGL(resize_bwd_kernel<bf16_t>, dim3(cdiv(total, 256)), dim3(256), 0, st, (const bf16_t*)dy, (long)dsw, (bf16_t*)dx, (long)xsw, B, H,
                       W, Ho, Wo, C);
  else
    hipLaunchKernelGGL(resize_bwd_kernel<float>, dim3(cdiv(total, 256)), dim3(256), 0, st, (const float*)dy, (long)dsw, (float*)dx, (long)xsw, B, H, W,
                       Ho, Wo, C);
  Y3D_LAUNCH_CHECK();
  return Y3D_OK;
}

}  // extern "C"
