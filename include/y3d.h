/* y3d.h — C ABI of liby3d_hip.so: the MI355X (gfx950) kernels of the YOLOv10 / YOLOv10-3D hot path.
 *
 * The reference (baldhat/yolov10-3D) has no native layer: every entry point below replaces a
 * *torch op call site* inside one of the reference's nn.Modules / loss functions (file:line cited
 * per function, paths relative to ultralytics/).  The host-side mirror of those modules
 * (yolov10-3d_amd/modules.py, loss.py) binds this library through ctypes; INTEGRATION.md shows the
 * binding a reference maintainer would add.
 *
 * Conventions
 *   - all tensors are device pointers; activations are NHWC ("channels last"): element (b,h,w,c) of a
 *     tensor with strides (sb, sh, sw) lives at  ptr + b*sb + h*sh + w*sw + c   (strides in ELEMENTS).
 *     "pixel-dense" tensors only carry `sw` (pixel stride; sh = W*sw, sb = H*W*sw) so they may be
 *     channel slices of a wider buffer (concat-free writes).
 *   - dtype: Y3D_F32 (exact-f32 MFMA / fp32 VALU; the parity mode) or Y3D_BF16 (bf16 storage + bf16 MFMA,
 *     fp32 accumulation / statistics / loss math; the performance mode).
 *   - 16-byte chunks: channel counts, channel offsets and strides of activation tensors must be
 *     multiples of 4 (f32) / 8 (bf16) elements unless a function says otherwise.
 *   - `stream` is a hipStream_t (NULL = default stream).  Nothing here allocates, frees or synchronises:
 *     every call is capturable into a hipGraph.
 *   - return value: Y3D_OK or a negative Y3D_ERR_*; y3d_last_error() gives the message
 *     (the host mirror raises it as a Python exception — the reference's error behaviour).
 */
#ifndef Y3D_H
#define Y3D_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { Y3D_F32 = 0, Y3D_BF16 = 1 };
enum { Y3D_OK = 0, Y3D_ERR_INVALID = -1, Y3D_ERR_HIP = -2 };

const char* y3d_last_error(void);
int y3d_abi_version(void);
/* name of the device the library would launch on, its CU count and LDS bytes per workgroup (sanity / roofline) */
int y3d_device_info(char* name, int name_len, int* compute_units, int* lds_bytes, int* clock_khz);

/* ------------------------------------------------------------------------------------------------
 * Dense / grouped convolution, implicit GEMM on MFMA (conv_gemm.hip)
 * replaces nn.Conv2d.forward + autograd backward at nn/modules/conv.py:115,120-122 (Conv),
 * head.py:633-637 (3D head branches), block.py:225-226,336-337 (C2f / Bottleneck), ...
 * ---------------------------------------------------------------------------------------------- */
/* OIHW fp32 parameter -> K-contiguous compute-dtype layout [Cout][kh*kw][Cin_g_pad] */
int y3d_pack_weight_fwd(int dtype, const float* w_oihw, void* out, int Cout, int Cin_g, int Cin_g_pad, int kh, int kw, void* stream);
/* OIHW fp32 parameter -> [G][Cin_g][kh*kw][Cout_g] (row pitch y3d_conv_kpad(dtype, kh*kw*Cout_g)) for the data gradient */
int y3d_pack_weight_dgrad(int dtype, const float* w_oihw, void* out, int Cout, int Cin_g, int groups, int kh, int kw, void* stream);
/* the two packings above for MANY weights in one launch (once per step, after the optimizer): desc is a DEVICE array of 8 int64 per
 * weight {src fp32 OIHW, dst, a, b, c, taps, Kpad, mode}; mode 0 = forward layout (a = Cout, b = Cin/g, c = padded Cin/g),
 * mode 1 = data-gradient layout (a = groups, b = Cout/g, c = Cin/g), mode 2 = the depth-wise layout of y3d_dw_pack_weight, always
 * fp32 (a = 1, b = C, c = 1, Kpad = taps * C); chunk tables as in the optimizer kernels below: a chunk is `chunk` consecutive
 * elements of a destination, and the workgroup it goes to packs the rows (of Kpad elements) that start in it */
int y3d_mt_pack_weights(int dtype, const int64_t* desc, const int* chunk_tensor, const int* chunk_off, int nchunks, int chunk, void* stream);
/* fp8 conv weights (fp8w.hip; BASELINE configs[4], no reference counterpart): OCP e4m3fn codes with one power-of-two scale per
 * output channel, scale = 2^ceil(log2(absmax / 448)).  MANY weights in one launch: desc is a DEVICE array of 6 int64 per weight
 * {src fp32 (rows, K), w_eff fp32 (rows, K) or 0, codes uint8 (rows, K) or 0, scale fp32 (rows), rows, K}, row_begin (ntensors) the
 * first global row of each weight, nrows their total.  w_eff = value(code) * scale is exactly representable in bf16, so the bf16
 * matrix-core kernels compute fp8-weight products exactly when they pack w_eff instead of the master weight. */
int y3d_mt_fp8w_quantize(const int64_t* desc, const int* row_begin, int ntensors, int nrows, void* stream);
/* codes (rows, K) + scale (rows) -> fp32 weights (loading a 1-byte-per-weight checkpoint) */
int y3d_fp8w_dequantize(const uint8_t* codes, const float* scale, float* w, int rows, int K, void* stream);
/* fp8 MFMA convolution family (conv3x3_fp8.hip; BASELINE configs[4], no reference counterpart): 3x3 stride-1 "same" conv FORWARD on
 * v_mfma_scale_f32_16x16x128_f8f6f4 with OCP-MX operands.
 *   y3d_fp8_quantize_act: bf16 NHWC rows x (M pixels, row stride xsw elements, C % 32 == 0) -> e4m3 codes q (M, C) + E8M0 block scales s
 *     (M, y3d_fp8_scale_pitch(C)): C / 32 bytes per pixel, rows padded to whole dwords; scale = the smallest power of two with
 *     amax(32 channels) / scale <= 448, code = RNE(x / scale) (never saturates);
 *   y3d_fp8_pack_weight_fwd: the fp8w quantiser's codes (rows, Cg * 9) in OIHW order + power-of-two row scales -> K-contiguous bytes
 *     wq (rows, 9, Cg) + E8M0 bytes ws (rows);
 *   y3d_conv3x3_fp8_fwd: y (bf16 NHWC, pixel stride ysw) = conv(x, w) with fp32 accumulation; training form: stat_partials
 *     [y3d_conv3x3_fp8_stat_rows][Cout][2] (sum, sum^2 of y as stored), eval form: y = act(conv * scale[c] + shift[c]).
 *     Served geometries: y3d_conv3x3_fp8_ok (Cin / groups a multiple of 64, at least 128; Cout / groups a multiple of 16). */
int y3d_fp8_quantize_act(const void* x, int64_t xsw, int64_t M, int C, uint8_t* q, uint8_t* s, void* stream);
int y3d_fp8_pack_weight_fwd(const uint8_t* codes, const float* scale, int rows, int Cg, uint8_t* wq, uint8_t* ws, void* stream);
int y3d_conv3x3_fp8_ok(int B, int H, int W, int Cin, int Cout, int groups);
int y3d_conv3x3_fp8_stat_rows(int B, int H, int W);
int y3d_fp8_scale_pitch(int C);
int y3d_conv3x3_fp8_fwd(const uint8_t* xq, const uint8_t* xs, int B, int H, int W, int Cin, const uint8_t* wq, const uint8_t* ws, void* y, int64_t ysw,
                        int Cout, int groups, float* stat_partials, const float* scale, const float* shift, int act, void* stream);
/* fp8 DATA GRADIENT of the same layers (opt-in: ops.set_fp8_dgrad).  dx of a 3x3 stride-1 pad-1 conv is that conv of dy with the taps
 * flipped and the channel roles swapped: the forward kernel runs on (dy, codes) in its plain-store form.  The fp8w row scales belong to
 * the REDUCTION index there; powers of two, they are folded exactly into dy before it is quantised:
 *   y3d_fp8_quantize_grad: y3d_fp8_quantize_act of dy[c] * scale[c] (fp32 product, exact): dy bf16 NHWC rows (M pixels, pixel stride sw,
 *     C % 32 == 0), scale (C) fp32 -> q (M, C) + s (M, y3d_fp8_scale_pitch(C));
 *   y3d_fp8_pack_weight_dgrad: the fp8w quantiser's codes (Cout, Cin / groups * 9), OIHW -> wq [groups][Cin / groups][9, flipped: t -> 8 - t]
 *     [(hi - lo) / groups] bytes for the output channels [lo, hi) (a window needs groups == 1) + ws (Cin) unit E8M0 bytes (127);
 *   y3d_conv3x3_fp8_dgrad: dx (bf16 NHWC, Cin channels, pixel stride dxsw) from channels [lo, hi) of dyq (rows qsw bytes wide) / dys (rows
 *     spitch bytes wide); lo % 128 == 0.  Served: y3d_conv3x3_fp8_dgrad_ok (Cout / groups a multiple of 64, >= 128; Cin / groups a
 *     multiple of 16; H >= 4, W >= 8) with Cout = hi - lo. */
int y3d_fp8_quantize_grad(const void* dy, int64_t sw, const float* scale, int64_t M, int C, uint8_t* q, uint8_t* s, void* stream);
int y3d_fp8_pack_weight_dgrad(const uint8_t* codes, int Cout, int Cin, int groups, int lo, int hi, uint8_t* wq, uint8_t* ws, void* stream);
int y3d_conv3x3_fp8_dgrad_ok(int B, int H, int W, int Cin, int Cout, int groups);
int y3d_conv3x3_fp8_dgrad(const uint8_t* dyq, const uint8_t* dys, int64_t qsw, int spitch, int lo, int hi, int B, int H, int W, const uint8_t* wq, const uint8_t* ws,
                          void* dx, int64_t dxsw, int Cin, int groups, void* stream);
int y3d_conv_kpad(int dtype, int k_total);
/* number of BatchNorm partial rows of the generic implicit-GEMM kernel: ceil(B*Ho*Wo / 128) */
int y3d_conv_stat_blocks(int B, int Ho, int Wo);
/* number of BatchNorm partial rows y3d_conv2d_fwd emits for this geometry (depends on the kernel it dispatches to:
 * 3x3 s1 p1 convs with 128-byte channel slabs run the resident-halo tile kernel, one row per TH x 16 pixel tile) */
int y3d_conv2d_stat_rows(int dtype, int B, int H, int W, int Cin, int Cout, int groups, int kh, int kw, int stride, int pad);
/* the kernel a convolution entry point launches for this geometry, with pixel-dense NHWC operands (a view that is not pixel-dense
 * can only move a 1x1 conv or a stride-2 data gradient off its streaming / resident kernel).  op: Y3D_OP_*; epi (forward only, else
 * 0): Y3D_EPI_*.  Returns a Y3D_ROUTE_* code, or Y3D_ERR_INVALID where the entry point refuses the geometry (y3d_last_error says
 * why).  y3d_conv2d_fwd / _fwd_affine / _fwd_affine_res, y3d_conv2d_bwd_data and y3d_conv2d_bwd_weight dispatch on this decision. */
enum { Y3D_OP_FWD = 0, Y3D_OP_BWD_DATA = 1, Y3D_OP_BWD_WEIGHT = 2 };
enum { Y3D_EPI_RAW = 0, Y3D_EPI_PARTIALS = 1, Y3D_EPI_AFFINE = 2, Y3D_EPI_AFFINE_RES = 3, Y3D_EPI_BIAS = 4 };
enum {
  Y3D_ROUTE_GENERIC = 0,          /* conv_gemm.hip: implicit GEMM (forward, data gradient) / split-K weight gradient */
  Y3D_ROUTE_STREAM1X1 = 1,        /* conv1x1_stream.hip */
  Y3D_ROUTE_SMALL = 2,            /* conv3x3_small.hip, stride 1 */
  Y3D_ROUTE_SMALL_S2 = 3,         /* conv3x3_small.hip, stride 2 (forward) */
  Y3D_ROUTE_S2_DGRAD = 4,         /* conv3x3s2_dgrad.hip */
  Y3D_ROUTE_TILE8 = 5,            /* conv3x3_tile.hip, 8-row tiles */
  Y3D_ROUTE_TILE16 = 6,           /* conv3x3_tile.hip, 16-row tiles */
  Y3D_ROUTE_WIDE3_8 = 7,          /* conv3x3_wide3.hip, 8-row tiles (also ragged heights) */
  Y3D_ROUTE_WIDE3_16 = 8,         /* conv3x3_wide3.hip, 16-row tiles */
  Y3D_ROUTE_FLAT = 9,             /* conv3x3_flat.hip */
  Y3D_ROUTE_WGRAD_SMALL = 10,     /* wgrad3x3_small.hip */
  Y3D_ROUTE_WGRAD_TILE = 11,      /* conv3x3_wgrad_tile.hip */
  Y3D_ROUTE_WGRAD_STREAM1X1 = 12  /* wgrad1x1_stream.hip */
};
int y3d_conv2d_route(int dtype, int op, int epi, int B, int H, int W, int Cin, int Cout, int groups, int kh, int kw, int stride, int pad);
/* y = conv(x, w) (+bias).  stat_partials (optional, no bias): [y3d_conv_stat_blocks][Cout][2] = per-block (sum, sum^2) of y. */
int y3d_conv2d_fwd(int dtype, const void* x, int64_t xsb, int64_t xsh, int64_t xsw, int B, int H, int W, int Cin,
                   const void* w_packed, const float* bias, void* y, int64_t ysw, int Ho, int Wo, int Cout, int groups,
                   int kh, int kw, int stride, int pad, float* stat_partials, void* stream);
/* eval-mode Conv in ONE launch: y = act(conv(x, w) * scale[c] + shift[c]) with scale/shift from y3d_bn_eval_scale
 * (Conv.forward with BatchNorm in eval mode, conv.py:120-122; equals the reference's fuse_conv_and_bn folding, torch_utils.py:171-198) */
int y3d_conv2d_fwd_affine(int dtype, const void* x, int64_t xsb, int64_t xsh, int64_t xsw, int B, int H, int W, int Cin,
                          const void* w_packed, const float* scale, const float* shift, int act, void* y, int64_t ysw, int Ho, int Wo,
                          int Cout, int groups, int kh, int kw, int stride, int pad, void* stream);
/* the same with the residual of a shortcut block added AFTER the activation: y = act(conv(x, w) * scale + shift) + res
 * (Bottleneck.forward in eval mode, block.py:342).  Only geometries for which y3d_conv2d_fwd_affine_res_ok returns 1 (bf16 3x3 s1 p1,
 * <= 64 input and output channels: the narrow resident-weight kernel); other callers run y3d_conv2d_fwd + y3d_bn_act_fwd. */
int y3d_conv2d_fwd_affine_res_ok(int dtype, int B, int H, int W, int Cin, int Cout, int groups, int kh, int kw, int stride, int pad);
int y3d_conv2d_fwd_affine_res(int dtype, const void* x, int64_t xsb, int64_t xsh, int64_t xsw, int B, int H, int W, int Cin,
                              const void* w_packed, const float* scale, const float* shift, int act, const void* res, int64_t rsw, void* y,
                              int64_t ysw, int Ho, int Wo, int Cout, int groups, int kh, int kw, int stride, int pad, void* stream);
/* dx = conv_transpose(dy, w)  (F.conv2d backward w.r.t. input) */
int y3d_conv2d_bwd_data(int dtype, const void* dy, int64_t dsb, int64_t dsh, int64_t dsw, int B, int Ho, int Wo, int Cout,
                        const void* w_packed_dgrad, void* dx, int64_t xsw, int H, int W, int Cin, int groups, int kh, int kw,
                        int stride, int pad, void* stream);
/* split-K factor of the generic weight-gradient kernel; slab must hold nsplit*Cout*kh*kw*Cin_g floats */
int y3d_conv2d_wgrad_splits(int dtype, int B, int Ho, int Wo, int Cout, int Cin_g, int groups, int kh, int kw);
/* split-K factor y3d_conv2d_bwd_weight expects for this geometry (it dispatches 3x3 s1 p1 bf16 convs with 64-channel slabs to
 * the resident-tile weight-gradient kernel); same slab sizing rule */
int y3d_conv2d_wgrad_plan(int dtype, int B, int H, int W, int Cin, int Cout, int groups, int kh, int kw, int stride, int pad);
/* testing / A-B knob: 0 routes every convolution through the generic implicit-GEMM kernels; returns the previous value */
int y3d_set_tile_kernels(int enable);
/* same for the streaming 1x1 kernels (conv1x1_stream.hip: bf16 1x1 stride-1 forward / data gradient, LDS-resident weights;
 * wgrad1x1_stream.hip: its weight gradient, LDS-DMA ring) */
int y3d_set_stream1x1(int enable);
int y3d_get_stream1x1(void);
int y3d_get_tile_kernels(void);
/* same for the row-wide workgroup slabs of the BatchNorm forward / backward-apply passes on bf16 tensors with >= 512 channels
 * (bn_act.hip: slab_width) */
int y3d_set_bn_wide_slabs(int enable);
/* same for the zero-skip of y3d_proj_group_bn_bwd (mode 0) and y3d_proj_group_bwd_weight_bn_mfma (proj_bn_mfma.hip): on (the default),
 * pixel chunks whose `dout` rows of a branch are all +0 skip that branch's dz / activation / MFMA work; off, every chunk takes the
 * dense path.  The results are bit-identical for finite inputs (the header of proj_bn_mfma.hip has the argument and the one difference) */
int y3d_set_proj_zero_skip(int enable);
/* grad_oihw (+)= dL/dw.  Cin may be channel-padded (stem): only the first Cin_real channels are written. */
int y3d_conv2d_bwd_weight(int dtype, const void* x, int64_t xsb, int64_t xsh, int64_t xsw, int B, int H, int W, int Cin,
                          int Cin_real, const void* dy, int64_t dsw, int Ho, int Wo, int Cout, int groups, int kh, int kw,
                          int stride, int pad, float* slab, int nsplit, float* grad_oihw, int accumulate, void* stream);
/* the last pass of y3d_conv2d_bwd_weight on its own: grad_oihw[co][ci][tap] (+)= sum over the nsplit slabs [co][tap][ci] (Cin_g
 * channels per tap, of which the first Cin_g_real are written), in the fixed order documented at wgrad_reduce_kernel */
int y3d_wgrad_fold(const float* slab, int nsplit, int Cout, int taps, int Cin_g, int Cin_g_real, float* grad_oihw, int accumulate,
                   void* stream);

/* ------------------------------------------------------------------------------------------------
 * Depth-wise convolution (dwconv.hip) — Conv(g=c): conv.py:172-177, block.py:705-706,747-751,783,824
 * ---------------------------------------------------------------------------------------------- */
int y3d_dw_blocks(int64_t M);        /* rows of BN partials for M output pixels */
int y3d_dw_wgrad_blocks(int64_t M);  /* weight-gradient slabs for M output pixels */
int y3d_dw_pack_weight(const float* w_oihw, float* out_taps_c, int C, int kh, int kw, void* stream);
int y3d_dwconv2d_fwd(int dtype, const void* x, int64_t xsb, int64_t xsh, int64_t xsw, int B, int H, int W, int C,
                     const float* w_packed, void* y, int64_t ysw, int Ho, int Wo, int kh, int kw, int stride, int pad,
                     float* stat_partials, void* stream);
/* eval: z = act(dwconv(x) * scale[c] + shift[c] (+ res, res_mode 2)) (+ res, res_mode 1) in one launch - the folded BatchNorm + SiLU (+ the
 * RepVGGDW / shortcut residual, block.py:711, 758) applied to the depth-wise result rounded as y3d_dwconv2d_fwd would have stored it, so the
 * values are those of y3d_dwconv2d_fwd + y3d_bn_act_fwd bit for bit */
int y3d_dwconv2d_fwd_affine(int dtype, const void* x, int64_t xsb, int64_t xsh, int64_t xsw, int B, int H, int W, int C,
                            const float* w_packed, const float* scale, const float* shift, int act, int res_mode, const void* res, int64_t rsw,
                            void* z, int64_t zsw, int Ho, int Wo, int kh, int kw, int stride, int pad, void* stream);
int y3d_dwconv2d_bwd_data(int dtype, const void* dy, int64_t dsb, int64_t dsh, int64_t dsw, int B, int Ho, int Wo, int C,
                          const float* w_packed, void* dx, int64_t xsw, int H, int W, int kh, int kw, int stride, int pad,
                          void* stream);
/* slab: y3d_dw_wgrad_blocks(B*Ho*Wo) * kh*kw*C floats */
int y3d_dwconv2d_bwd_weight(int dtype, const void* x, int64_t xsb, int64_t xsh, int64_t xsw, int B, int H, int W, int C,
                            const void* dy, int64_t dsw, int Ho, int Wo, int kh, int kw, int stride, int pad, float* slab,
                            float* grad_oihw, int accumulate, void* stream);
/* its last pass on its own: grad_oihw[c][tap] (+)= sum over the nblk slabs [tap][c] */
int y3d_dw_wgrad_fold(const float* slab, int nblk, int C, int taps, float* grad_oihw, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * BatchNorm (batch or running statistics) + SiLU + residual (bn_act.hip)
 * replaces nn.BatchNorm2d / nn.SiLU / `x + ...` at conv.py:106,118-122, block.py:342,711,758,816-817;
 * eps / momentum semantics of utils/torch_utils.py:327-337
 * ---------------------------------------------------------------------------------------------- */
/* partials [nblk][C][2] -> mean, invstd, scale = gamma*invstd, shift = beta - mean*scale; running stats
 * updated in place (momentum, unbiased variance) when running_mean != NULL */
int y3d_bn_finalize(const float* partials, int nblk, int C, int64_t count, const float* gamma, const float* beta, float eps,
                    float momentum, float* running_mean, float* running_var, float* mean, float* invstd, float* scale,
                    float* shift, void* stream);
int y3d_bn_eval_scale(int C, const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                      float eps, float* scale, float* shift, void* stream);
/* u = y*scale+shift (+res if res_mode==2); z = act ? silu(u) : u; (+res if res_mode==1) */
int y3d_bn_act_fwd(int dtype, const void* y, int64_t ysw, const float* scale, const float* shift, int act, int res_mode,
                   const void* res, int64_t rsw, void* z, int64_t zsw, int64_t P, int C, void* stream);
/* y3d_bn_act_fwd (bf16, no residual, C % 64 == 0) that ALSO writes the fp8 copy of z the next layer's fp8 MFMA convolution reads:
 * q (P, C) e4m3 codes + s (P, y3d_fp8_scale_pitch(C)) E8M0 block scales, exactly what y3d_fp8_quantize_act makes of z */
int y3d_bn_act_fwd_q(const void* y, int64_t ysw, const float* scale, const float* shift, int act, void* z, int64_t zsw, uint8_t* q, uint8_t* s,
                     int64_t P, int C, void* stream);
int y3d_bn_bwd_blocks(int64_t P, int C);
/* pass 1: partials [y3d_bn_bwd_blocks(P, C)][C][2] = (sum g, sum g*xhat), g = dz * act'(u) */
int y3d_bn_act_bwd_reduce(int dtype, const void* y, int64_t ysw, const void* dz, int64_t dsw, const void* res, int64_t rsw,
                          const float* scale, const float* shift, const float* mean, const float* invstd, int act,
                          int res_mode, float* partials, int64_t P, int C, void* stream);
/* dgamma/dbeta (+)= sums; mean_g, mean_gx = sums / count */
int y3d_bn_bwd_finalize(const float* partials, int nblk, int C, int64_t count, float* dgamma, float* dbeta, int accumulate,
                        float* mean_g, float* mean_gx, void* stream);
/* pass 2: dy = scale*(g - mean_g - xhat*mean_gx) [train] or scale*g [eval]; dres = g for res_mode==2 */
int y3d_bn_act_bwd_apply(int dtype, const void* y, int64_t ysw, const void* dz, int64_t dsw, const void* res, int64_t rsw,
                         const float* scale, const float* shift, const float* mean, const float* invstd,
                         const float* mean_g, const float* mean_gx, int act, int res_mode, int train, void* dy, int64_t dysw,
                         void* dres, int64_t drsw, int64_t P, int C, void* stream);
/* column sums of a [P][C] tensor as partials [y3d_bn_bwd_blocks(P, C)][C][2] (bias gradients; reduce with y3d_bn_bwd_finalize) */
int y3d_colsum_partials(int dtype, const void* x, int64_t xsw, float* partials, int64_t P, int C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Graph glue (misc.hip)
 * ---------------------------------------------------------------------------------------------- */
/* nn.MaxPool2d(k, 1, k//2) — SPPF block.py:171-178.  argmax: [B*H*W][C] uint8 tap index (may be NULL) */
int y3d_maxpool_fwd(int dtype, const void* x, int64_t xsb, int64_t xsh, int64_t xsw, void* y, int64_t ysw, uint8_t* argmax,
                    int B, int H, int W, int C, int k, void* stream);
int y3d_maxpool_bwd(int dtype, const void* dy, int64_t dsw, const uint8_t* argmax, void* dx, int64_t xsw, int B, int H, int W,
                    int C, int k, void* stream);
/* nn.Upsample(None, 2, "nearest") — cfg/models/v10 and v10-3D yaml rows; x is (B,H,W,C), y is (B,2H,2W,C) */
int y3d_upsample2x_fwd(int dtype, const void* x, int64_t xsb, int64_t xsh, int64_t xsw, void* y, int64_t ysw, int B, int H, int W,
                       int C, void* stream);
int y3d_upsample2x_bwd(int dtype, const void* dy, int64_t dsb, int64_t dsh, int64_t dsw, void* dx, int64_t xsw, int B, int H,
                       int W, int C, void* stream);
/* torch.cat(dim=1) member copy — Concat conv.py:404, block.py:178,233,818: y[:, :C] = x over P pixels */
int y3d_copy2d(int dtype, const void* x, int64_t xsw, void* y, int64_t ysw, int64_t P, int C, void* stream);
/* diagnostic, no reference counterpart (tools/cu_contention.py): n workgroups that stay resident on `stream` until *flag != 0 (device
 * int) or ~50 ms, moving a trickle of data inside buf - a stand-in for an RCCL kernel's CU footprint next to the backward pass */
int y3d_occupy_cus(int n, const int* flag, float* buf, int64_t nbuf, void* stream);
int y3d_add2d(int dtype, const void* a, int64_t asw, const void* b, int64_t bsw, void* y, int64_t ysw, int64_t P, int C, void* stream);
/* model boundary: reference tensors are NCHW fp32 (nn/tasks.py:93-95) */
int y3d_nchw_to_nhwc(int dtype, const float* x_nchw, void* y_nhwc, int B, int C, int H, int W, int Cpad, void* stream);
/* stem (nn/tasks.py yaml row 0: Conv(3, c, 3, 2)): NCHW fp32 image -> [B][Ho][Wo][32], column (r*3+q)*3+ci of the 3x3 stride-2 pad-1
 * window, columns 27..31 zero; the stem conv is then y3d_conv2d_fwd / _bwd_weight with a 1x1 kernel over 32 channels */
int y3d_stem_im2col(int dtype, const float* x_nchw, void* out, int B, int H, int W, int Ho, int Wo, void* stream);
/* the same from the dataset's uint8 image (NCHW: hwc = 0, NHWC as decoded: hwc = 1) with the /255 of data/datasets/kitti.py:204-205
 * (models/yolo/detect/train.py:59 for the 2D trainer) done on the device: 1 byte per sample crosses PCIe / HBM instead of 4 */
int y3d_stem_im2col_u8(int dtype, const uint8_t* x, int hwc, void* out, int B, int H, int W, int Ho, int Wo, void* stream);
/* the eval stem in one pass - Conv(3, Cout, 3, 2) with running-statistics BatchNorm folded into (scale, shift) and SiLU (act != 0),
 * nn/modules/conv.py:120-122 on yaml row 0: x = (B, 3, H, W) fp32 (in_mode 0), (B, 3, H, W) uint8 (1) or (B, H, W, 3) uint8 (2; uint8
 * samples are divided by 255 as data/datasets/kitti.py:204-205); wcol = [Cout][32] fp32 with column (r*3+q)*3+ci of the 3x3 window
 * (27..31 zero); y = bf16 (B, Ho, Wo) pixels x Cout channels (16, 32, 48, 64 or 80), pixel pitch ysw elements.  bf16 arithmetic as
 * y3d_stem_im2col + y3d_conv2d_fwd_affine, without the column tensor. */
int y3d_stem_conv_eval(const void* x, int in_mode, const float* wcol, const float* scale, const float* shift, int act, void* y, int64_t ysw,
                       int B, int H, int W, int Cout, void* stream);
/* the training stem in one pass: the same gather + MFMA writing the raw conv output y (bf16, before BatchNorm), the column tensor
 * xcol = [B*Ho*Wo][32] bf16 that y3d_stem_im2col would have produced (operand of the weight gradient) and BatchNorm partials
 * part[rows][Cout][2] (sum, sum of squares of the stored values; rows = y3d_stem_conv_train_rows) for y3d_bn_finalize -
 * replaces y3d_stem_im2col + y3d_conv2d_fwd (K = 32), which wrote the column tensor and read it back */
int y3d_stem_conv_train_rows(int B, int H, int W);
int y3d_stem_conv_train(const void* x, int in_mode, const float* wcol, void* y, int64_t ysw, void* xcol, float* part, int B, int H, int W,
                        int Cout, void* stream);
int y3d_nhwc_to_nchw(int dtype, const void* x_nhwc, int64_t xsw, float* y_nchw, int B, int C, int H, int W, void* stream);
/* head final nn.Conv2d(c, out, 1) with bias, out <= 24 — head.py:637 (3D branches: nc,2,2,2,3,24,1,1) */
int y3d_proj_fwd(int dtype, const void* x, int64_t xsw, const float* w, const float* bias, void* y, int64_t ysw, int64_t P,
                 int Cin, int Cout, void* stream);
int y3d_proj_bwd_data(int dtype, const void* dy, int64_t dsw, const float* w, void* dx, int64_t xsw, int64_t P, int Cin, int Cout,
                      void* stream);
int y3d_proj_blocks(int64_t P);
/* slab: y3d_proj_blocks(P)*Cout*Cin floats, bias_slab: y3d_proj_blocks(P)*Cout floats */
int y3d_proj_bwd_weight(int dtype, const void* x, int64_t xsw, const void* dy, int64_t dsw, float* slab, float* bias_slab,
                        float* grad_w, float* grad_b, int accumulate, int64_t P, int Cin, int Cout, void* stream);
int y3d_slab_reduce(const float* slab, float* out, int nblk, int64_t n, int accumulate, void* stream);
/* the nb (<= 16) final projections of one head level in ONE launch (proj_group.hip): branch j reads channels
 * [xoff[j], xoff[j]+cin) of x and writes couts[j] channels at the running output offset (the torch.cat of head.py:742).
 * w / b / dw / db: host arrays of nb device pointers.  slab: y3d_proj_group_blocks(P)*sum(couts)*cin floats, bslab: ...*sum(couts) */
int y3d_proj_group_fwd(int dtype, int nb, int cin, const void* x, int64_t xsw, const int* xoff, const float* const* w,
                       const float* const* b, const int* couts, void* y, int64_t ysw, int64_t P, void* stream);
int y3d_proj_group_bwd_data(int dtype, int nb, int cin, const void* dy, int64_t dsw, const int* xoff, const float* const* w,
                            const int* couts, void* dx, int64_t xsw, int64_t P, void* stream);
/* BatchNorm backward of the conv that feeds a projection group, recomputing dz = dout . W on the matrix cores instead of reading a
 * materialised gradient tensor (proj_bn_mfma.hip, bf16, cin = 64 / 128; the backward of head.py:633-637 + conv.py:120 for one level):
 * mode 0: partials [y3d_proj_group_bn_bwd_blocks(P)][C][2] = (sum g, sum g*xhat), g = dz * act'(u)  -> y3d_bn_bwd_finalize;
 * mode 1: dy = scale * (g - mean_g - xhat * mean_gx).  y_pre: the conv's pre-BatchNorm output (C channels, branch i at xoff[i]),
 * dout: gradient of the projected map (branch i's couts[i] channels side by side in branch order). */
/* the forward of the same stage on the matrix cores (bf16, cin = 64 / 128): out[px][branch i's channels] = W_i . act(y_pre * scale + shift) + b_i */
int y3d_proj_group_fwd_bn_mfma(int nb, int cin, const void* y_pre, int64_t ysw, const int* xoff, const float* const* w, const float* const* b,
                               const int* couts, const float* scale, const float* shift, int act, void* out, int64_t osw, int64_t P,
                               void* stream);
/* ... and its weight / bias gradients (contraction over pixels; transposed LDS reads): slab = blocks * sum(couts) * cin floats,
 * bslab = blocks * sum(couts) floats, blocks = y3d_proj_group_bwd_weight_bn_mfma_blocks(P) */
int y3d_proj_group_bwd_weight_bn_mfma_blocks(int64_t P);
int y3d_proj_group_bwd_weight_bn_mfma(int nb, int cin, const void* y_pre, int64_t ysw, const int* xoff, const void* dout, int64_t dsw,
                                      const int* couts, const float* scale, const float* shift, int act, float* slab, float* bslab,
                                      float* const* dw, float* const* db, int64_t P, void* stream);
int y3d_proj_group_bn_bwd_blocks(int64_t P);
int y3d_proj_group_bn_bwd(int mode, int nb, int cin, const void* y_pre, int64_t ysw, const int* xoff, const void* dout, int64_t dsw,
                          const float* const* w, const int* couts, const float* scale, const float* shift, const float* mean,
                          const float* invstd, const float* mean_g, const float* mean_gx, int act, float* partials, int nblk, void* dy,
                          int64_t dysw, int64_t P, int C, void* stream);
int y3d_proj_group_blocks(int64_t P);
/* the same projections fused with the BatchNorm (+SiLU) that precedes them: y_pre is the PRE-BatchNorm conv output; the activation
 * act(y_pre * scale + shift) is formed on the fly (forward) / rebuilt (weight gradient) and never stored */
int y3d_proj_group_fwd_bn(int dtype, int nb, int cin, const void* y_pre, int64_t xsw, const int* xoff, const float* const* w,
                          const float* const* b, const int* couts, const float* scale, const float* shift, int act, void* out,
                          int64_t ysw, int64_t P, void* stream);
int y3d_proj_group_bwd_weight_bn(int dtype, int nb, int cin, const void* y_pre, int64_t xsw, const int* xoff, const void* dy, int64_t dsw,
                                 const int* couts, const float* scale, const float* shift, int act, float* slab, float* bslab,
                                 float* const* dw, float* const* db, int64_t P, void* stream);
int y3d_proj_group_bwd_weight(int dtype, int nb, int cin, const void* x, int64_t xsw, const int* xoff, const void* dy, int64_t dsw,
                              const int* couts, float* slab, float* bslab, float* const* dw, float* const* db, int64_t P, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PSA attention core (attn.hip) — Attention.forward block.py:785-797
 * qkv: (B, N, nh*(2kd+hd)) with per-head block [q|k|v]; out: (B, N, nh*hd); lse/delta: (B, nh, N) fp32
 * ---------------------------------------------------------------------------------------------- */
int y3d_attn_fwd(int dtype, const void* qkv, int64_t qsw, void* out, int64_t osw, float* lse, int B, int N, int nh, int kd, int hd,
                 float scale, void* stream);
int y3d_attn_bwd(int dtype, const void* qkv, int64_t qsw, const void* out, int64_t osw, const void* dout, int64_t dsw,
                 const void* dv_extra, int64_t esw, const float* lse, float* delta, void* dqkv, int64_t gsw, int B, int N, int nh,
                 int kd, int hd, float scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 3D task-aligned assignment + 3D detection loss (tal_loss3d.hip)
 * replaces TaskAlignedAssigner3d.forward utils/tal.py:392-452 (+ keypoint_utils.py:11-118, metrics.py:78-134) and
 * DDDetectionLoss.__call__ utils/loss.py:821-963 for one head set.
 * maps[l]: (B, H[l], W[l], >= nc+35) NHWC head map of level l (pointer at channel 0 of the head set, pixel stride psw[l]);
 * anchors are level-major, row-major (tal.py:300-312).  gt: (B, n, 17) padded targets of loss.py:795-810
 * (cls | box xyxy px | center_2d | size_2d | center_3d | size_3d | depth | heading_bin | heading_res).
 * ---------------------------------------------------------------------------------------------- */
int y3d_tal3d_scratch_floats(int B, int n, int A, int topk);
/* `preprocess` utils/loss.py:795-810 (3D: :848-856, 2D: :223-226): rows (nbox, 1+width) = [batch_idx | cls | box xywh in [0,1] | ...] ->
 * out (B, cap, width) zero-padded per image in order of appearance, box scaled by (scale_x, scale_y) and converted to xyxy px.
 * n_used: TWO device ints.  n_used[0] = min(largest per-image box count, cap): the assigners take it as a DEVICE pointer, so —
 * unlike the reference's host-side `counts.max()` — padding the targets needs no host synchronisation.  n_used[1] = the largest
 * count itself: boxes beyond `cap` per image are dropped, and a caller must treat n_used[1] > cap as an error (loss.pad_targets
 * reads it back asynchronously and raises). */
int y3d_pad_targets(const float* rows, int nbox, int width, int B, int cap, float scale_x, float scale_y, float* out, int* n_used,
                    void* stream);
/* outputs: fg_mask (B,A) uint8, target_gt_idx (B,A) int32, target_scores (B,A,nc) fp32 (normalised),
 * scal[0] = max(sum(target_scores), 1), scal[1] = number of foreground anchors.
 * n = rows per image of gt (capacity, <= 64); n_used: device int from y3d_pad_targets (rows >= *n_used are padding in every
 * image and are skipped), or NULL = all n rows are walked.  The results do not depend on n_used. */
/* mode (cfg/default.yaml:116-119 -> utils/tal.py:465-497): bit 0 `tal_2d` (box metric), bit 1 `tal_3d` (keypoint metric; at least one of
 * the two), bit 2 `kps_dist_metric: l2` (else l1), bit 3 `constrain_anchors` (candidates inside the box only).  Default 1 | 2 | 8 = 11. */
int y3d_tal3d_assign(int dtype, int nl, const void* const* maps, const int64_t* psw, const int* H, const int* W, const float* strides,
                     int B, int nc, const float* gt, int n, const float* calib, const float* mean_sizes, int topk, float alpha,
                     float beta, float gamma, int mode, float* scratch, uint8_t* fg_mask, int* target_gt_idx, float* target_scores, float* scal,
                     const int* n_used, void* stream);
/* items[6] = (box2d, cls, depth, offset3d, size3d, heading) of loss.py:886-891; grads[l] (pixel stride gsw[l]) receives
 * grad_scale * d(sum(items))/d(map) for all nc+35 channels.  partials: 6 * ceil(B*A/256) floats */
int y3d_loss3d(int dtype, int nl, const void* const* maps, const int64_t* psw, void* const* grads, const int64_t* gsw, const int* H,
               const int* W, const float* strides, int B, int nc, const float* gt, int n, const uint8_t* fg_mask,
               const int* target_gt_idx, const float* target_scores, const float* scal, float w_loss2d, float w_cls, float w_depth,
               float w_offset3d, float w_size3d, float w_heading, float grad_scale, float* partials, float* items, void* stream);
/* y3d_loss3d with device-side item weights (hierarchical task learning, engine/trainer.py:398-400).  item_w: 6 device floats in the
 * order of items[].  Every gradient channel belongs to one item - class logits: cls; nc+0..3: box2d; nc+4..5: offset3d; nc+6..8: size3d;
 * nc+9..32: heading; nc+33..34: depth - and is stored as (d(item)/d(map) * grad_scale) * item_w[item].  items[6] stay UNWEIGHTED by
 * item_w, exactly as y3d_loss3d writes them; total[0] = (float) sum_j (double)item_w[j] * (double)items[j], j ascending.
 * grads == NULL: no gradient row is stored (a pass under no_grad).  Nothing is read back: item_w may change between two launches. */
int y3d_loss3d_weighted(int dtype, int nl, const void* const* maps, const int64_t* psw, void* const* grads, const int64_t* gsw, const int* H,
                        const int* W, const float* strides, int B, int nc, const float* gt, int n, const uint8_t* fg_mask,
                        const int* target_gt_idx, const float* target_scores, const float* scal, float w_loss2d, float w_cls, float w_depth,
                        float w_offset3d, float w_size3d, float w_heading, float grad_scale, float* partials, float* items,
                        const float* item_w, float* total, void* stream);
/* Hierarchical task learning, utils/htl.py:23-56 `compute_weight` on device state (htl.hip): one launch of one workgroup, fp32, in the
 * reference's operation order.  items: the current 12 loss items (one-to-many set first); time_value = min((epoch - 5) / (T - 5), 1),
 * computed by the caller in double.  State: ring (stat_epochs x 12 floats, oldest first) with its fill count, init_diff[12] with its
 * have_init flag, weights[12] (output: w / sum(w) * 6), status (bit 0 is SET, never cleared, when a weight or the sum is not finite).
 * stat_epochs in 3..8.  The current items enter the ring after the weights were computed. */
int y3d_htl_update(const float* items, float time_value, int stat_epochs, float* ring, int* count, float* init_diff, int* have_init,
                   float* weights, int* status, void* stream);

/* Feature distillation, utils/loss.py:1156-1188 SupervisionLoss.forward_head as called at :893-898, for one head set (distill.hip).
 * embs[l]: (B, H[l], W[l], >= C) NHWC slice of the depth branch's first-layer output at level l (pointer at its channel 0, pixel
 * stride psw[l] elements, dtype `dtype`); C % 8 == 0.  teacher: (B, C, th, tw) of `teacher_dtype` with element strides (tsb, tsc, tsh,
 * tsw): NCHW and NHWC are both accepted.  gt: the (B, n, 17) padded targets; fg_mask / target_gt_idx / scal: outputs of
 * y3d_tal3d_assign (scal[0] = max(sum(target_scores), 1)); mixed: (B) uint8 or NULL when no_mixup == 0.  criterion: 0 soft, 1 mse,
 * 2 cos.  An image takes part when it has a valid box and is not (no_mixup and mixed).  The teacher row of an anchor is read at
 * round-half-even(center_3d / (img_w, img_h) * (tw, th)) of padded row target_gt_idx, clamped to the map: the valid rows of an image
 * must be a prefix of its n rows (y3d_pad_targets lays them out so).  An image with boxes but no foreground anchor contributes 0 (the
 * reference: NaN).
 * Outputs: loss[0] = the item as the reference stores it in loss[6] (weighted, divided by scal[0]); the COMPACT gradient of loss[0]
 * wrt the embeddings: row r (C values of `dtype`) belongs to image idx[2r], anchor idx[2r+1] (level-major, row-major), rows ordered by
 * (image, anchor); counts[0..B) = foreground anchors per participating image (else 0), counts[B] = rows written = min(total, cap),
 * counts[B+1] = total.  cap = row capacity: B*n*topk bounds the assigner's foreground set.  counts: B+2 ints, idx: 2*cap ints,
 * rows: cap*C elements, partials: ceil(cap/4) floats.  No float atomics: the results are the same bits on every run. */
int y3d_distill_loss(int dtype, int nl, const void* const* embs, const int64_t* psw, const int* H, const int* W, int B, int C,
                     const void* teacher, int teacher_dtype, int th, int tw, int64_t tsb, int64_t tsc, int64_t tsh, int64_t tsw,
                     const float* gt, int n, const uint8_t* fg_mask, const int* target_gt_idx, const float* scal, const uint8_t* mixed,
                     int img_w, int img_h, float T, float weight, int criterion, int no_mixup, int cap, int* counts, int* idx,
                     void* rows, float* partials, float* loss, void* stream);
/* grad[b, y, x, 0..C) += scale[0] * row r for every row of y3d_distill_loss whose anchor lies in the level that starts at anchor a0
 * (H x W pixels); grad: pointer at the slice's channel 0 with element strides (sb, sh, sw) of image / row / pixel; scale: device fp32. */
int y3d_distill_scatter(int dtype, const void* rows, const int* idx, const int* nrows, const float* scale, int cap, int C, void* grad,
                        int64_t sb, int64_t sh, int64_t sw, int a0, int H, int W, void* stream);

/* Foreground depth map loss, utils/loss.py:1225-1365 ForegroundDepthMapLoss (focal_loss / one_hot :1399-1522), fgdm_loss.hip.
 * logits: (B, num_bins + 1, h, w) of `dtype` with element strides (sb, sc, sh, sw): contiguous and channels_last are both just strides.
 * depth_map: dense (B, H, W) float32 (map_f64 == 0) or float64 (map_f64 != 0); (h, w) must be (H / 16, W / 16).  Cell (b, i, j) samples
 * the map at ATen's nearest-exact index, bins the depth with the LID rule in float64 (class num_bins for out-of-range, non-finite and
 * background depths), and takes sum_c (delta_ct + 1e-6) * -alpha (1 - p_c)^gamma log p_c, weighted fg_weight where the depth is > 0,
 * else bg_weight.  loss[0] = sum of the weighted cell losses / (B h w); dlogits (the logits' dtype and strides) = d loss / d logits.
 * partials: y3d_fgdm_loss_blocks(B, h, w) floats, folded in a fixed order (no float atomics: the same bits on every run).
 * targets: NULL, or B*h*w ints that receive every cell's class (a debug output).  num_bins <= 255; gamma == 0 or gamma >= 1. */
int y3d_fgdm_loss_blocks(int B, int h, int w);
int y3d_fgdm_loss(int dtype, const void* logits, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int map_f64, const void* depth_map, int B,
                  int H, int W, int h, int w, int num_bins, double dmin, double dmax, float alpha, float gamma, float fg_weight,
                  float bg_weight, void* dlogits, float* partials, float* loss, int* targets, void* stream);
/* dst[i] = src[i] * scale[0] for n elements of `dtype` (16-byte aligned, dense, not overlapping); scale: device fp32 */
int y3d_fgdm_scale(int dtype, const void* src, const float* scale, void* dst, int64_t n, void* stream);

/* 2D counterparts (tal_loss2d.hip): TaskAlignedAssigner utils/tal.py:45-94 and v8DetectionLoss utils/loss.py:206-257 (+BboxLoss :82-113,
 * DFL block.py:59-62).  maps[l]: (B, H, W, 64 + nc) with channel order [4 x 16 DFL bins | nc class logits]; gt: (B, n, 5) = cls | box xyxy px.
 * scratch as y3d_tal3d_scratch_floats.  items[3] = (box, cls, dfl) incl. gains; partials: 3 * ceil(B*A/256) floats */
int y3d_tal2d_assign(int dtype, int nl, const void* const* maps, const int64_t* psw, const int* H, const int* W, const float* strides,
                     int B, int nc, const float* gt, int n, int topk, float alpha, float beta, float* scratch, uint8_t* fg_mask,
                     int* target_gt_idx, float* target_scores, float* scal, const int* n_used, void* stream);
int y3d_loss2d(int dtype, int nl, const void* const* maps, const int64_t* psw, void* const* grads, const int64_t* gsw, const int* H,
               const int* W, const float* strides, int B, int nc, const float* gt, int n, const uint8_t* fg_mask,
               const int* target_gt_idx, const float* target_scores, const float* scal, float w_box, float w_cls, float w_dfl,
               float grad_scale, float* partials, float* items, void* stream);
/* Crowded route of the 2D assigner: 1 <= n <= 512 rows per image, same arguments and the same outputs as y3d_tal2d_assign (fg_mask and
 * target_gt_idx bit for bit), without a buffer that grows with n * A: each box looks only at the grid cells under it and the anchors
 * resolve by claim counts.  scratch: y3d_tal2d_scratch_floats(B, n, A, topk) floats, 16-byte aligned =
 * B * n * 42 + 7 * B * A + 2 * ceil(B * A / 256) + 8, or -1 past 2^31.  loss.Loss2dFn takes this route when n > 64 (`max_boxes`). */
int y3d_tal2d_scratch_floats(int B, int n, int A, int topk);
int y3d_tal2d_assign_crowded(int dtype, int nl, const void* const* maps, const int64_t* psw, const int* H, const int* W, const float* strides,
                             int B, int nc, const float* gt, int n, int topk, float alpha, float beta, float* scratch, uint8_t* fg_mask,
                             int* target_gt_idx, float* target_scores, float* scal, const int* n_used, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Eval-side selection (post.hip): v10Detect3d.select_candidates / extract_patches / scatter / decode (head.py:656-716,
 * 755-797) and v10_3Dpostprocess / v10postprocess (utils/ops.py:852-880).  Ties go to the lowest index.
 * ---------------------------------------------------------------------------------------------- */
/* out_idx (B, K) int32: flat cell index (row*W + col) of the K largest max-class logits of each image; cls: (B, HW, >= nc), pixel stride psw */
int y3d_topk_cells(int dtype, const void* cls, int64_t psw, int B, int HW, int nc, int K, int* out_idx, void* stream);
/* out (B*K, ps, ps, C) NHWC: zero-padded ps x ps input patches centred on the selected cells */
int y3d_patch_gather(int dtype, const void* x, int64_t xsb, int64_t xsh, int64_t xsw, const int* idx, void* out, int B, int H, int W,
                     int C, int K, int ps, void* stream);
/* map (B, HW, no): dense cls channels + the (no - nc) regression channels of the candidate on each selected cell, zeros elsewhere */
int y3d_head3d_scatter(int dtype, const void* cls, int64_t csw, const void* reg, int64_t rsw, const int* idx, void* map, int B, int HW,
                       int nc, int no, int K, void* stream);
/* y (B, nc+35, A) fp32 from the per-level (B, H, W, nc+35) maps: xyxy px boxes, centre-3d px, the rest copied */
int y3d_head3d_decode(int dtype, int nl, const void* const* maps, const int* H, const int* W, const float* strides, int B, int nc,
                      float* y, void* stream);
/* 2D head decode — Detect.inference head.py:53-79 (DFL softmax expectation block.py:59-62, dist2bbox(xywh) tal.py:315-325, sigmoid):
 * maps[l] (B, H, W, 64 + nc) NHWC pixel-dense with channels [4 x 16 box-side bins | nc class logits] -> y (B, 4 + nc, A) fp32 =
 * (cx, cy, w, h) px | scores */
int y3d_head2d_decode(int dtype, int nl, const void* const* maps, const int* H, const int* W, const float* strides, int B, int nc,
                      float* y, void* stream);
/* y (B, C, A) fp32; scores are the first nc rows (3D, boxes_first = 0) or the last nc rows (2D, boxes_first = 1).
 * reg (B, max_det, C-nc), scores (B, max_det), labels (B, max_det) int64 */
int y3d_v10_postprocess_scratch_floats(int B, int A, int nc, int max_det); /* 0 when the score row fits LDS, else B*A */
int y3d_v10_postprocess(const float* y, int B, int C, int A, int nc, int max_det, int boxes_first, float* reg, float* scores,
                        int64_t* labels, float* scratch, void* stream);

/* Input pipeline, image side of KITTIDataset.__getitem__ (data/datasets/kitti.py:132-206): mirror (:149, :184), mixup blend
 * `Image.blend(img, img2, 0.5)` (:188), affine crop `img.transform(resolution, AFFINE, trans_inv, BILINEAR)` (:192-196) in
 * Pillow's arithmetic (bit-exact: double-precision mapping of pixel centres, clamped bilinear taps, truncation), `/255` (:204).
 * src / src2: DEVICE arrays of B device pointers to (H, W, 3) uint8 RGB images (src2 entries or src2 itself may be NULL: no mixup);
 * hw (B, 2) int32 source sizes, flip (B) int32, trans_inv (B, 6) float64 (output -> source), all on the device.
 * mode 0: out (B, 3, out_h, out_w) fp32 = the reference's tensor; mode 1: out (B, out_h, out_w, 3) uint8 (feeds y3d_stem_im2col_u8,
 * which divides by 255 itself). */
int y3d_kitti_image_aug(const unsigned char* const* src, const unsigned char* const* src2, const int* hw, const int* flip, const double* trans_inv,
                        int B, int out_h, int out_w, int mode, void* out, void* stream);
/* One-to-many depth fusion of the 3D validator — YOLOv10_3DDetectionValidator.aggregate_o2m_preds models/yolov10_3D/val.py:78-102:
 * predsO (B, K, C), predsM (B, KM, C) post-processed rows [xyxy | ... | depth (C-4) | depth log-variance (C-3) | score | label (C-1)];
 * the one-to-many rows with IoU > iou_thres, the same label and exp(-log-variance) > thres vote on the depth through a weighted
 * gaussian kernel density (silverman bandwidth as scikit-learn defines it), evaluated at nprop float32 proposals between the
 * extreme votes; out (B, K, C) = predsO with the most likely proposal as depth.  KM <= 3902: the votes of one detection are kept in
 * 64 KiB of LDS; more is an error and nothing is written. */
int y3d_kde_depth_fusion(const float* predsO, int B, int K, const float* predsM, int KM, int C, float thres, float iou_thres, int nprop,
                         float* out, void* stream);
/* Depth of the 3D validator's rows from a supplied depth map — YOLOv10_3DDetectionValidator.dino_depth_pred models/yolov10_3D/val.py:61-76:
 * rows (B, K, C) post-processed rows [xyxy | centre-3d x (4), y (5), network-input pixels | ... | depth (C-4) | ...], map (B, Hm, Wm),
 * all fp32; out (B, K, C) = rows with column C-4 replaced by map[b, iy, ix], ix = column 4 truncated toward zero and clamped to
 * [0, Wm-1], iy the same from column 5 and Hm.  The clamp is done in float BEFORE the conversion: !(c >= 0) -> 0, c >= dim -> dim-1, so a
 * NaN reads index 0 and a huge value the last index (the reference's `.long()` is undefined for both).  C >= 8, no empty size, out must
 * not overlap rows or map, no NULL: otherwise an error and nothing is written. */
int y3d_rows_depth_from_map(const float* rows, int B, int K, int C, const float* map, int Hm, int Wm, float* out, void* stream);
/* KITTI decode of the post-processed detections (data/datasets/kitti.py:519-576 `decode_preds`, called by the validator's
 * `_prepare_preds`, models/yolov10_3D/val.py:210-214).  preds (B, K, 37) fp32 rows [xyxy | centre-3d | size residual | 24 heading |
 * depth | depth log-variance | score logit | label]; calib (B, 6) = (cu, cv, fu, fv, tx, ty) of the original image; ratio (B, 2) =
 * ratio_pad[i][0]; inv_trans (B, 2, 3) or NULL (undo_augment = False: the fixed 1242/1280, 375/384 rescale); mean_size (nc, 3).
 * out (B, K, 14) f64 [cls, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, score]; keep (B, K) u8 = !(score < threshold). */
int y3d_kitti_decode(const float* preds, int B, int K, const double* calib, const double* ratio, const double* inv_trans,
                     const double* mean_size, int nc, int use_camera_dis, double threshold, double* out, unsigned char* keep, void* stream);
/* Input pipeline, label side of KITTIDataset.__getitem__ (data/datasets/kitti.py:208-405) and its collate_fn (:579-599), one workgroup
 * per image (kitti_labels.hip).  rec (N, 16) float64 label records, images back to back, each image's primary lines then its mixup
 * partner's, in label-file order: [cls id (0 .. n_cls-1, -1 for any other type), truncation, occlusion, x1, y1, x2, y2 (float32
 * values), h, w, l, pos x, y, z (float32 values), ry, 0].  img_i (B, 7) int32 = (primary start row, primary line count, partner start
 * row, partner line count (0: no mixup), flip, original width, original height); img_f (B, 19) float64 = P2 (3x4, already flipped
 * when flip, float32 values), trans (2x3, original -> output), crop scale.  Outputs in a static layout of max_objs (<= 64) rows per
 * image, survivors first in the reference's order, the rest batch_idx = -1 and zeros: cls (B*max_objs) int64, bboxes (.., 4) f64
 * xywh / resolution clipped to [0, 1], center_2d (.., 2) f32, size_2d (.., 2) f32, center_3d (.., 2) f64, size_3d (.., 3) f64,
 * depth f64, heading_bin int64, heading_res f64, batch_idx f32; counts (B) int32; calib (B, 6) f64 = (cu, cv, fu, fv, tx, ty) x the
 * resolution ratio; ratio_pad (B, 2, 2) f64. */
int y3d_kitti_encode_labels(const double* rec, const int* img_i, const double* img_f, int B, int out_w, int out_h, double min_depth,
                            double max_depth, int use_camera_dis, const double* mean_size, int n_cls, int max_objs, int64_t* cls,
                            double* bboxes, float* center_2d, float* size_2d, double* center_3d, double* size_3d, double* depth,
                            int64_t* heading_bin, double* heading_res, float* batch_idx, int* counts, double* calib, double* ratio_pad,
                            void* stream);
/* y3d_kitti_encode_labels (the same kernel, the same outputs bit for bit) that also writes the per-line depth table of the foreground
 * depth map: line_depth (B, 2, 64) float32, [b][0][i] = the depth label line i of image b's own file paints (the float32 rounding of
 * pos z * crop scale, never the camera distance), [b][1][i] = the same for the mixup partner's line i; +inf for a line that is
 * dropped by the filter chain, lies behind the max_objs cut or does not exist. */
int y3d_kitti_encode_labels_depths(const double* rec, const int* img_i, const double* img_f, int B, int out_w, int out_h, double min_depth,
                                   double max_depth, int use_camera_dis, const double* mean_size, int n_cls, int max_objs, int64_t* cls,
                                   double* bboxes, float* center_2d, float* size_2d, double* center_3d, double* size_3d, double* depth,
                                   int64_t* heading_bin, double* heading_res, float* batch_idx, int* counts, double* calib,
                                   double* ratio_pad, float* line_depth, void* stream);
/* Foreground depth maps, `load_depth_maps` of KITTIDataset.__getitem__ (data/datasets/kitti.py:143-145, 170-201, 286-287, 384-385,
 * 409-417), kitti_depth_map.hip.  A mask is (h, w) uint8, a pixel = the label-file line index of its object (ids above 255 stored as
 * 255).  Masks either as per-image device pointers `mask` / `mask2` (B each; the partner's entry NULL for an unmixed image, mask2 NULL
 * when no image is mixed) with arena == NULL, or as one `arena` with mask_off (N) int64 byte offsets and the device draw table
 * `draws` (B, draw_w) float64 whose columns 0 / 1 hold the position and the partner (-1: none); then mask == mask2 == NULL.  wide: NULL,
 * or uint8 flags of the masks that came from 16-bit files (Pillow warps an I;16 image by a path of its own): (B, 2) own | partner
 * with mask pointers, (N) per frame with an arena.  hw (B, 2) int32 (h, w) of the masks, flip (B) int32, trans_inv (B, 6) float64: the tables of y3d_kitti_image_aug; max_side: the largest mask
 * side (refused from 32768).  out (B, out_h, out_w) float32: per pixel the source pixel of Pillow's Image.transform(AFFINE, NEAREST,
 * fillcolor=51) over the mirrored mask - its scale path (a[1] == a[3] == 0: running double sums) or its 16.16 fixed-point path for an
 * 8-bit mask, its generic double-precision path for a 16-bit one - then min(line_depth[b][0][id], line_depth[b][1][partner id]) (ids >= 64 match nothing), 0 where that exceeds max_depth or
 * nothing matches.  xy: B * (out_w + out_h) ints of workspace (the scale path's column / row tables, made by a launch of B blocks). */
int y3d_kitti_depth_map(const unsigned char* const* mask, const unsigned char* const* mask2, const unsigned char* arena, const int64_t* mask_off,
                        const double* draws, int draw_w, const unsigned char* wide, const int* hw, const int* flip, const double* trans_inv,
                        const float* line_depth, int B, int out_h, int out_w, int max_side, double max_depth, int* xy, float* out,
                        void* stream);
/* Batch plan over a KITTI split held on the device (kitti_cache.hip, kitti.DeviceSplit), one thread per image: the per-image tables of
 * y3d_kitti_image_aug and y3d_kitti_encode_labels from the split's frame tables and one table of draws.  Frame tables, on the device,
 * indexed by dataset position (N frames): img_off (N) int64 byte offsets into arena (every frame (H, W, 3) uint8 RGB); frame_hw (N, 2)
 * int32 (H, W); rec_span (N, 2) int32 = (first row, line count) in the split's label records; P2 (N, 2, 12) float32 = the calibration
 * as read and the one of the mirrored image.  draws (B, 16) float64 on the device, draws_host the same table in host memory:
 * [position, mixup partner or -1, flip, crop scale, trans (6), trans_inv (6)]; positions and partners outside [0, N) are refused from
 * draws_host before the launch.  Outputs, on the device: src / src2 (B) pointers = arena + img_off (src2: NULL without a partner), hw
 * (B, 2), flip (B) int32, trans_inv (B, 6) as y3d_kitti_image_aug takes them; img_i (B, 7) = (first row, lines, partner's first row,
 * partner's lines, flip, W, H) and img_f (B, 19) = (P2[position][flip] widened, trans, scale) as y3d_kitti_encode_labels takes them,
 * the rows counted in the split's records; mixed (B) uint8. */
int y3d_kitti_plan_batch(const int64_t* img_off, const int* frame_hw, const int* rec_span, const float* P2, int N,
                         const unsigned char* arena, const double* draws_host, const double* draws, int B, const unsigned char** src,
                         const unsigned char** src2, int* hw, int* flip, double* trans_inv, int* img_i, double* img_f,
                         unsigned char* mixed, void* stream);
/* Input pipeline, label side of WaymoDataset.__getitem__ (data/datasets/waymo.py:186-290, load_object :292-372; dataset = 0) and
 * Omni3Dataset.__getitem__ (data/datasets/omni3d.py:175-279, load_object :281-352; dataset = 1) with their collate_fn, one workgroup
 * per image (json3d_labels.hip), in the plan and the output layout of y3d_kitti_encode_labels.  rec (N, 24) float64 object records,
 * images back to back, each image's primary objects then its mixup partner's, in annotation order: [cls id (0 .. n_cls-1, -1 for any
 * other category), x1, y1, x2, y2 (float32 values), h, w, l, pos x, y, z (the bottom-face centre), ry, num_lidar, behind_camera,
 * valid3D, depth_error, truncation, visibility, 0 ...] (the five after num_lidar are read for Omni3D only).  img_i (B, 7) and img_f
 * (B, 19) as y3d_kitti_encode_labels takes them, but P2 holds the float64 calibration of the JSON when the image is not mirrored and
 * the float32 values of Calibration.flip when it is.  Waymo's 2D box is recomputed from the projected corners of the 3D box
 * (recompute_bbox_2d, waymo.py:365-372), Omni3D's is the annotated one; mean_size (n_cls, 3) is the dataset's table. */
int y3d_json3d_encode_labels(const double* rec, const int* img_i, const double* img_f, int B, int dataset, int out_w, int out_h,
                             double min_depth, double max_depth, int use_camera_dis, const double* mean_size, int n_cls, int max_objs,
                             int64_t* cls, double* bboxes, float* center_2d, float* size_2d, double* center_3d, double* size_3d,
                             double* depth, int64_t* heading_bin, double* heading_res, float* batch_idx, int* counts, double* calib,
                             double* ratio_pad, void* stream);
/* Width of a row of y3d_json3d_plan_batch's draw table (float64 values). */
enum { Y3D_JSON3D_DRAW_W = 18 };
/* Batch plan over a Waymo / Omni3D split held in two tiers (json3d_cache.hip, json3d.DeviceSplit), one thread per image: the tables of
 * y3d_kitti_plan_batch, for y3d_kitti_image_aug and y3d_json3d_encode_labels.  The frames at positions [0, n_dev) live in `arena` on
 * the device, those at [n_dev, N) in pinned host memory; the ones a batch uses have been copied into `stage`, a device buffer of
 * stage_bytes bytes, by the time this kernel runs.  Frame tables, on the device, indexed by dataset position: img_off (N) int64 byte
 * offsets into arena, -1 at [n_dev, N) and never read there; frame_hw (N, 2) int32 (H, W); rec_span (N, 2) int32 = (first row, object
 * count) in the split's records, a frame without annotations has a zero-length span at the running row; P2 (N, 2, 12) float64 = the
 * calibration as read and the float32 one of the mirrored image, widened.  draws (B, Y3D_JSON3D_DRAW_W) float64 on the device,
 * draws_host the same table in host memory: the sixteen columns of y3d_kitti_plan_batch, then the byte offset into stage of the
 * primary's frame and of the partner's, -1 for a frame of the arena.  Refused from draws_host before the launch, nothing written: a
 * position or partner that is no integer of [0, N) (partner: or -1); an offset other than -1 for a position below n_dev, or for no
 * partner; for a position from n_dev on, an offset that is -1, negative, no integer multiple of 16 or not below stage_bytes.  arena
 * may be NULL when n_dev == 0, stage when no row names an offset.  Outputs as y3d_kitti_plan_batch's: src / src2 = stage + offset or
 * arena + img_off; img_f[:12] is a plain copy of P2[position][flip]. */
int y3d_json3d_plan_batch(const int64_t* img_off, const int* frame_hw, const int* rec_span, const double* P2, int N, int n_dev,
                          const unsigned char* arena, const unsigned char* stage, int64_t stage_bytes, const double* draws_host,
                          const double* draws, int B, const unsigned char** src, const unsigned char** src2, int* hw, int* flip,
                          double* trans_inv, int* img_i, double* img_f, unsigned char* mixed, void* stream);
/* 2D input pipeline, image side of YOLODataset.__getitem__ (data/base.py load_image :147-182; data/augment.py Mosaic._mosaic4
 * :208-242, RandomPerspective :384-435, MixUp :337-344, RandomHSV :605-624, RandomFlip :651-681, Format._format_img :950-957) for a
 * batch, one launch (yolo2d_batch.hip states the arithmetic; float64, + - * / and floor only).  src: DEVICE table of n_src device
 * pointers to decoded (H, W, 3) uint8 images.  rec_i (B, 112) int32: two layers (the sample, its MixUp partner) of [tiles, canvas
 * side, 4 x (src index, h0, w0, resized h, w, x1a, y1a, x2a, y2a, padw, padh, 0)], then at 100: flipud, fliplr, bgr, hsv, mix.
 * rec_f (B, 16) float64: the two layers' inverse matrices (2x3, output -> canvas), the MixUp ratio r.  lut (B, 3, 256) uint8: the
 * hue / saturation / value tables.  imgsz: a multiple of 4.  mode 0: out (B, 3, imgsz, imgsz) fp32 in [0, 1]; mode 1: out
 * (B, imgsz, imgsz, 3) uint8 (feeds y3d_stem_im2col_u8). */
int y3d_yolo2d_image_aug(const unsigned char* const* src, int n_src, const int* rec_i, const double* rec_f, const unsigned char* lut, int B,
                         int imgsz, int mode, void* out, void* stream);
/* 2D input pipeline, label side of the same sample (Mosaic._update_labels / _cat_labels :292-323, RandomPerspective.apply_bboxes /
 * box_candidates :437-460, :562-581, the flips, Format) and collate_fn (data/dataset.py:206-223), one workgroup per image.  rec
 * (n_rec, 5) float32 label rows [cls, x, y, w, h] normalised.  lab_i (B, 20) int32: (first row, rows) of the eight tiles (mosaic tiles
 * 0..3, then the partner's), the two layers' flags (bit 0 present, bit 1 mosaic: canvas clip + zero-area filter, bit 2 training: warp +
 * box_candidates + flips), flips (bit 0 up-down, bit 1 left-right), 0.  lab_f (B, 48) float32: (w, h, padw, padh) of the eight tiles,
 * then per layer (M 2x3, scale, 0).  Outputs in a static layout of cap (64, 128 .. 512) rows per image, survivors first in the
 * reference's order, the rest batch_idx = -1 and zeros: cls (B*cap) f32, bboxes (B*cap, 4) f32 xywh normalised, batch_idx f32;
 * counts (B) int32 = the true number of survivors, which may exceed cap (the surplus is not stored). */
int y3d_yolo2d_encode_labels(const float* rec, int n_rec, const int* lab_i, const float* lab_f, int B, int imgsz, int cap, float* cls,
                             float* bboxes, float* batch_idx, int* counts, void* stream);
/* Width of a row of y3d_yolo2d_plan_batch's draw table (float64 values). */
enum { Y3D_YOLO2D_DRAW_W = 56 };
/* Batch plan over a 2D split held on the device (yolo2d_cache.hip, yolo2d.DeviceSplit), one workgroup per sample: the five record
 * arrays of y3d_yolo2d_image_aug and y3d_yolo2d_encode_labels from the split's frame tables and one table of draws.  Frame tables, on
 * the device, indexed by dataset position (N frames): frame_hw (N, 2) int32 (h0, w0); rec_span (N, 2) int32 = (first row, rows) in the
 * split's label rows.  draws (B, Y3D_YOLO2D_DRAW_W) float64 on the device, draws_host the same table in host memory.  A row: two layers
 * of 23 (the sample, its MixUp partner): [present, mosaic, warp, frame position of tiles 0..3 (-1: none; one tile without mosaic), yc,
 * xc, canvas side, M 2x3 (float32 values), M_inv (6), scale]; then at 46: mix, r, hsv, the three HSV gains, flipud, fliplr, bgr, 0.
 * Positions of used tiles outside [0, N), and a sample without its first layer, are refused from draws_host before the launch.  The
 * kernel derives load_image's resized size, the mosaic rectangles or the letter-box placement and the pads from frame_hw and imgsz
 * (yolo2d_cache.hip states the arithmetic), and the HSV tables from the gains.  Outputs, on the device, in the layouts stated above:
 * rec_i (B, 112) int32 with source index = dataset position, rec_f (B, 16) float64, lut (B, 3, 256) uint8 (4-byte aligned; zeros
 * without the hsv flag), lab_i (B, 20) int32 with rows counted in the split's label rows, lab_f (B, 48) float32.  Every element of the B
 * rows is written.  Neither allocates nor synchronises. */
int y3d_yolo2d_plan_batch(const int* frame_hw, const int* rec_span, int N, int imgsz, const double* draws_host, const double* draws, int B,
                          int* rec_i, double* rec_f, unsigned char* lut, int* lab_i, float* lab_f, void* stream);
/* Rectangular letter-box of decoded images into one (H, W) canvas, H != W allowed (letterbox.hip states the arithmetic): the image side
 * of a rect=True validation sample (data/base.py load_image :147-182 + data/augment.py LetterBox.__call__ :696-742, Format._format_img
 * :950-957) and of the predictor's preprocess (engine/predictor.py:115-156).  src_table: DEVICE table of n_src device pointers to
 * decoded (h0, w0, 3) uint8 images, as y3d_yolo2d_image_aug takes it.  rec (B, 8) int32 = [src index, h0, w0, new_h, new_w, top, left,
 * swap_rb]: the source resized to (new_h, new_w) (a plain copy when that is (h0, w0)) lands at (top, left), everything else is 114;
 * swap_rb exchanges channels 0 and 2.  W: a multiple of 4.  mode 0: out (B, 3, H, W) fp32 in [0, 1]; mode 1: out (B, H, W, 3) uint8
 * (feeds y3d_stem_im2col_u8).  A record whose source index is outside the table or whose sizes are below 1 gives an all-114 image. */
int y3d_letterbox_image(const unsigned char* const* src_table, int n_src, const int* rec, int B, int H, int W, int mode, void* out,
                        void* stream);
/* Label side of a rect=True validation sample: LetterBox._update_labels (data/augment.py:744-750) + Format (:915-948) + collate_fn
 * (data/dataset.py:206-223), float32, one workgroup per image.  rec (n_rec, 5) float32 label rows [cls, x, y, w, h] normalised; lab_i
 * (B, 2) int32 = [first row, rows]; lab_f (B, 4) float32 = [w, h, padw, padh]: the resized image's size and the fractional pads dw, dh.
 * xywh -> xyxy, x (w, h), + (padw, padh), -> xywh, x (1/W, 1/H); no filter.  Outputs in the layout of y3d_yolo2d_encode_labels: cap
 * (64, 128 .. 512) rows per image in file order, the rest batch_idx = -1 and zeros; counts (B) int32 = the true number of rows. */
int y3d_letterbox_labels(const float* rec, int n_rec, const int* lab_i, const float* lab_f, int B, int H, int W, int cap, float* cls,
                         float* bboxes, float* batch_idx, int* counts, void* stream);
/* The predictor's row work (models/yolov10/predict.py:23-35; utils/ops.py scale_boxes :107-124, clip_boxes :127-145), one workgroup
 * per image.  preds (B, K, 6) fp32 [x1, y1, x2, y2, conf, cls] in the letter-boxed frame (v10postprocess + xywh2xyxy); meta (B, 5) fp32
 * = [h0, w0, gain, padw, padh].  A row is kept when conf > `conf` (strict) and, when n_cls > 0, its class equals one of classes (n_cls)
 * int32 (NULL when n_cls = 0).  Kept rows: x = (x - padw) / gain clipped to [0, w0], y = (y - padh) / gain clipped to [0, h0], fp32 with
 * IEEE division.  out (B, K, 6): the kept rows first, in input order, the rest zeros (out must not be preds); counts (B) int32. */
int y3d_predict_rows(const float* preds, const float* meta, float conf, const int* classes, int n_cls, int B, int K, float* out, int* counts,
                     void* stream);
/* The 3D predictor's row pass (predict3d.hip), one workgroup per image: KITTI decode, confidence / class filter, ordered compaction,
 * the eight box corners and their projection.  preds (B, K, 37) fp32, calib (B, 6), ratio (B, 2), inv_trans (B, 2, 3) or NULL,
 * mean_size (nc, 3), use_camera_dis: as y3d_kitti_decode takes them, and every kept row's 14 values are that kernel's bit for bit.
 * P2 (B, 12): the full 3 x 4 projection of the original image, float32 values promoted to double.  A row is kept when
 * !(score < conf) and, when n_cls > 0, (int)preds[.., 36] equals one of classes (n_cls) int32 (NULL when n_cls = 0).  For the j-th
 * kept row of image b, in input order: rows[b, j, 0:14] f64 [cls, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, score];
 * corners3d[b, j, 8, 3] f64, camera coordinates, Object3d.generate_corners3d's order (kitti_utils.py:98-114; y is the bottom face);
 * corners_img[b, j, 8, 2] f64 = Calibration.corners3d_to_img_boxes' boxes_corner (kitti_utils.py:266-284; the division is done
 * whatever its sign).  Slots j >= counts[b] of all three are zeros; counts (B) int32.  No output may overlap an input or
 * another output: the entry compares the byte ranges and refuses. */
int y3d_predict3d_rows(const float* preds, int B, int K, const double* calib, const double* P2, const double* ratio,
                       const double* inv_trans, const double* mean_size, int nc, int use_camera_dis, double conf, const int* classes,
                       int n_cls, double* rows, double* corners3d, double* corners_img, int* counts, void* stream);
/* The labels of a batch back to 3D boxes (decode_labels.hip): KITTIDataset.decode_batch (data/datasets/kitti.py:469-513, the same in
 * waymo.py and omni3d.py) with the corners and projection of y3d_predict3d_rows, one single-wave workgroup per image.  Per-box inputs,
 * N rows each, in the dtypes of y3d_kitti_encode_labels: cls int64, bboxes (N, 4) f64 xywh in [0, 1], center_3d (N, 2) f64,
 * size_3d (N, 3) f64 residuals, depth f64, heading_bin int64, heading_res f64, batch_idx f32.  Layout: with counts_in (B) int32 the static
 * one (N = B * max_objs, image b owns rows [b * max_objs, b * max_objs + min(counts_in[b], max_objs)); batch_idx is not read); with
 * counts_in NULL the ragged one of collate_fn (image b owns the rows with batch_idx == b, in batch order; N may be 0).
 * Per image: ori_shape (B, 2) f64 (height, width); calib (B, 6) = (cu, cv, fu, fv, tx, ty) of the original image; ratio = ratio_pad
 * as (B, 2, 2) (ratio_pitch 4) or (B, 2) (ratio_pitch 2); trans_inv (B, 2, 3) or NULL; P2 (B, 12) or NULL (then corners_img is NULL
 * too and nothing is projected).  undo_augment: the centre goes through trans_inv (rounded to float32 first, as affine_transform
 * does), which must then be given; otherwise it is divided by the ratio.  mean_size (nc, 3).
 * For the j-th owned row of image b, j < R: rows[b, j, 0:14] f64 [cls, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, 1]; corners3d
 * [b, j, 8, 3] and corners_img [b, j, 8, 2] as y3d_predict3d_rows writes them.  counts[b] = min(owned rows, R); slots behind are zeros.
 * A class outside [0, nc) stays in column 0 and takes the nearest table entry's size, as y3d_kitti_decode treats it.  The entry
 * refuses NULL or misaligned outputs (16 bytes; counts 4), R < 1, and any output whose byte range overlaps an input's or another
 * output's.  It neither allocates nor synchronises. */
int y3d_decode_labels(const int64_t* cls, const double* bboxes, const double* center_3d, const double* size_3d, const double* depth,
                      const int64_t* heading_bin, const double* heading_res, const float* batch_idx, const int* counts_in, int N, int max_objs,
                      int B, const double* ori_shape, const double* calib, const double* ratio, int ratio_pitch, const double* trans_inv,
                      const double* P2, const double* mean_size, int nc, int use_camera_dis, int undo_augment, int R, double* rows,
                      double* corners3d, double* corners_img, int* counts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Drawing 3D predictions (draw3d.hip; plot.py): box wireframes over the camera image and filled boxes on a bird's-eye-view map, the
 * pictures of KITTIVisualizer.plot_preds / plot_bev (utils/plotting.py:1280-1411) with exact coverage rules in place of OpenCV's
 * anti-aliased strokes.  All geometry is f64 with FMA contraction off, every sum evaluated left to right as written; pixel (x, y) is
 * the point (x, y).  Within one call the primitive with the LOWER index wins a pixel; a primitive with a non-finite coordinate is
 * skipped; the result depends on the inputs alone.  No entry allocates or synchronises.
 *   segment a -> b, thickness t, r2 = (t/2)(t/2), pixel p: d = b - a, e = p - a, len2 = d.x d.x + d.y d.y, dot = e.x d.x + e.y d.y;
 *     dot <= 0: covered iff e.x e.x + e.y e.y <= r2; dot >= len2: the same with p - b; else c = d.x e.y - d.y e.x, covered iff
 *     c c <= r2 len2 (no division, no square root; len2 == 0 is a disc).
 *   quad q0..q3: E_i = (q_{i+1} - q_i) x (p - q_i) = d_i.x (p.y - q_i.y) - d_i.y (p.x - q_i.x); covered iff all four E_i >= 0 or all
 *     four <= 0.  A quad with (q1 - q0) x (q2 - q0) + (q2 - q0) x (q3 - q0) == 0 (its doubled signed area) is skipped.
 * The raster kernels are exact for coordinates up to 1e12 in magnitude.
 * ---------------------------------------------------------------------------------------------- */
/* corners3d (B, K, 8, 3), rows (B, K, 14), counts (B) as y3d_predict3d_rows writes them; P2 (B, 12); affine (B, 6) or NULL; palette
 * (n_pal, 3) u8 -> segs (B, K * 14, 4) f64 [ax, ay, bx, by], seg_rgb (B, K * 14, 4) u8 [r, g, b, 0].  Box k owns slots k * 14 + j,
 * j = bottom face 0-1 1-2 2-3 3-0, top face 4-5 5-6 6-7 7-4, uprights 0-4 1-5 2-6 3-7, front-face diagonals 0-5 1-4.  Per endpoint
 * U = ((P0 x + P1 y) + P2 z) + P3 (V, W from rows 1, 2 of P2); both W < near_w: dropped; one W < near_w: that endpoint A becomes
 * A + s (B - A) in (U, V, W), s = (near_w - W_A) / (W_B - W_A); u = U / W, v = V / W; then u' = (A00 u + A01 v) + A02,
 * v' = (A10 u + A11 v) + A12.  Dropped segments and every slot of a box k >= counts[b] are NaN (those boxes' colours 0).  Colour:
 * palette[clamp((int)rows[b, k, 0], 0, n_pal - 1)], a NaN class taking entry 0; rows may be NULL (every box takes entry 0).  K may be 0. */
int y3d_box3d_segments(const double* corners3d, const double* rows, const int* counts, int B, int K, const double* P2, const double* affine,
                       const unsigned char* palette, int n_pal, double near_w, double* segs, unsigned char* seg_rgb, void* stream);
/* -> quads (B, K, 4, 2) f64: the bottom face's corners 0..3 as (cx + scale x, cy - scale z); quad_rgb (B, K, 4) u8 as above */
int y3d_box3d_bev_quads(const double* corners3d, const double* rows, const int* counts, int B, int K, const unsigned char* palette,
                        int n_pal, double scale, double cx, double cy, double* quads, unsigned char* quad_rgb, void* stream);
/* canvas (B, H, W, 3) u8, contiguous, painted in place: only covered pixels are stored.  Image b takes its first min(nseg[b], S)
 * segments (all S with nseg NULL) of segs (B, S, 4) / seg_rgb (B, S, 4).  thickness finite and > 0.  The canvas may overlap no input. */
int y3d_draw_segments(unsigned char* canvas, int B, int H, int W, const double* segs, const unsigned char* seg_rgb, const int* nseg, int S,
                      double thickness, void* stream);
/* the same with filled convex quads: quads (B, Q, 4, 2) f64, quad_rgb (B, Q, 4) u8, nquad (B) or NULL */
int y3d_draw_quads(unsigned char* canvas, int B, int H, int W, const double* quads, const unsigned char* quad_rgb, const int* nquad, int Q,
                   void* stream);

/* ------------------------------------------------------------------------------------------------
 * KITTI AP evaluation (kitti_eval.hip) — the evaluator behind KITTIDataset.get_stats (data/datasets/kitti.py:444-450):
 * eval_from_scrach / get_official_eval_result (data/datasets/kitti_eval.py:1268-1336, :1075-1165).
 * Boxes are packed per image, images back to back: gt / dt (N, 16) fp32 records
 *   [x1, y1, x2, y2, x, y, z, l, h, w, ry, alpha, score, occluded, truncated, 0]   (camera frame, y = bottom face)
 * gt_off / dt_off (n_img + 1) int32 prefix offsets into them; ov_off (n_img + 1) int64 prefix offsets of the per-image (n_dt, n_gt)
 * overlap blocks.  gt_code / dt_code (N) int32 name codes: 0 car, 1 pedestrian, 2 cyclist, 3 van, 4 person_sitting, 5 tractor,
 * 6 trailer, 7 other (case-insensitive), + 8 for a name that is exactly "DontCare".  At most y3d_kitti_eval_max_boxes() gts and dets
 * per image (the host layer checks; larger images are skipped by the kernels).  All arithmetic fp32, FMA contraction off.
 * ---------------------------------------------------------------------------------------------- */
int y3d_kitti_eval_max_boxes(void);
/* calculate_iou_partly(dt_annos, gt_annos, metric) (kitti_eval.py:698-781), the per-image blocks only: out[ov_off[i] + j * n_gt + g] =
 * overlap of det j with gt g of image i.  metric 0: image_box_overlap (:429-455); 1: bev_box_overlap / devRotateIoUEval over
 * (x, z, l, w, ry) with gt as rbox1 (:248-260, :458-461); 2: box3d_overlap with z_axis = 1, z_center = 1.0 (:465-515) */
int y3d_kitti_box_overlaps(int metric, const float* gt, const float* dt, const int* gt_off, const int* dt_off, const int64_t* ov_off,
                           int n_img, float* out, void* stream);
/* Threshold pass of eval_class_v3 (kitti_eval.py:868-883): compute_statistics_jit(compute_fp = False, thresh = 0) (:518-636) for every
 * (class x difficulty, min-overlap, image), ignore flags from clean_data (:369-425).  cd (ncd, 2) int32 = (class code, difficulty 0-2);
 * min_ov (ncd * nk) float64, setting s = cd_index * nk + k.  tp_score (ncd * nk, total_gt): the score of the det each gt is a true
 * positive of (entries of other gts are left as they are); nvalid (ncd, n_img): the image's gts with ignored_gt == 0 */
int y3d_kitti_eval_thresholds(const float* gt, const int* gt_code, const float* dt, const int* dt_code, const int* gt_off, const int* dt_off,
                              const int64_t* ov_off, const float* ov, int n_img, int total_gt, int metric, const int* cd, int ncd,
                              const double* min_ov, int nk, float* tp_score, int* nvalid, void* stream);
/* Counting pass: fused_compute_statistics (kitti_eval.py:648-696) — compute_statistics_jit(compute_fp = True) at the thresholds
 * thr (ncd * nk, 41) fp32, nthr (ncd * nk) of them per setting (get_thresholds :347-366), DontCare suppression for metric 0, AOS
 * similarity when compute_aos.  Work space cnt (ncd * nk * 41 * n_img * 3) int32, sim (ncd * nk * 41 * n_img) float64;
 * pr (ncd * nk, 41, 4) float64 = [tp, fp, fn, similarity] summed over images in a fixed order (bit-reproducible) */
int y3d_kitti_eval_counts(const float* gt, const int* gt_code, const float* dt, const int* dt_code, const int* gt_off, const int* dt_off,
                          const int64_t* ov_off, const float* ov, int n_img, int metric, const int* cd, int ncd, const double* min_ov, int nk,
                          const float* thr, const int* nthr, int compute_aos, int* cnt, double* sim, double* pr, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Validator box metrics (det_metrics.hip): P, R, mAP50, mAP50-95 — box_iou (utils/metrics.py:53), match_predictions with
 * use_scipy = False (engine/validator.py:229-273), the validators' box preparation (models/yolo/detect/val.py:97-175,
 * models/yolov10_3D/val.py:114-187) and ap_per_class / compute_ap (utils/metrics.py:532, :499).  fp32 boxes and IoU with FMA
 * contraction off; fp64 recall / precision / AP.  A tp mask holds bit t = "correct at thr[t]".  At most y3d_det_metrics_max_gts() gts
 * and y3d_det_metrics_max_dets() detections per image, at most 16 thresholds.
 * ---------------------------------------------------------------------------------------------- */
int y3d_det_metrics_max_gts(void);
int y3d_det_metrics_max_dets(void);
/* out (n1, n2) fp32 = IoU of box1[i] and box2[j], both (n, 4) xyxy fp32 */
int y3d_box_iou(const float* box1, int n1, const float* box2, int n2, float eps, float* out, void* stream);
/* one image: iou (n_gt, n_det) fp32, gt_cls (n_gt) / det_cls (n_det) int32, thr (n_thr) fp32 > 0 -> tp (n_det) int32 masks */
int y3d_match_predictions(const float* iou, const int* gt_cls, int n_gt, const int* det_cls, int n_det, const float* thr, int n_thr,
                          int* tp, void* stream);
/* One validation batch, one workgroup per image.  mode 0 (2D): preds (B, K, 6) fp32 [x1, y1, x2, y2, conf, cls] in the letterboxed
 * (img_h, img_w) frame, meta (B, 5) f64 [h0, w0, gain, padw, padh] (ori_shape, ratio_pad); mode 1 (3D): preds (B, K, 14) f64
 * decode_preds_eval rows (cls col 0, box cols 2:6, score col 13), meta (B, 2) f64 [h0, w0].  keep (B, K) u8 or NULL (all rows).
 * Targets as collated: gt_img / gt_cls (n_gt) fp32 batch_idx / cls, gt_box (n_gt, 4) fp32 normalised xywh.  Row (b, k) writes slot
 * b * K + k of tp (int32 mask), conf (f64) and cls (int32; -1 for a row that is not kept).  An image with more gts than the limit is
 * scored without gts and atomicMax's its gt count into status[0]. */
int y3d_box_match_batch(int mode, const void* preds, const unsigned char* keep, int B, int K, const double* meta, int img_h, int img_w,
                        int single_cls, const float* gt_img, const float* gt_cls, const float* gt_box, int n_gt, const float* thr,
                        int n_thr, int* tp, double* conf, int* cls, int* status, void* stream);
/* ConfusionMatrix.process_batch (utils/metrics.py:319-376) for one validation batch, one workgroup per image: the batch arguments of
 * y3d_box_match_batch (the same box preparation and fp32 IoU, bit for bit), nc classes, a row takes part iff kept and its confidence
 * > conf (strict; fp32 for mode 0, f64 for mode 1), pairs with iou > (float)iou_thres (strict, >= 0) are matched by two argmax passes
 * whatever their classes (ties: the higher gt index, then the higher detection index).  ADDS into matrix (nc + 1, nc + 1) int32,
 * [predicted, true], index nc = background, with integer atomics.  An image without gts adds nothing (neither validator calls
 * process_batch for it); an image without a single match does not count its detections (the reference's `if n:`).  K may be 0 (every
 * gt is missed).  status (2) int32: [0] atomicMax of the gt count of an image above the limit (it adds nothing), [1] set when a
 * class outside [0, nc) was met (that box is not counted). */
int y3d_confusion_batch(int mode, const void* preds, const unsigned char* keep, int B, int K, const double* meta, int img_h, int img_w,
                        int single_cls, const float* gt_img, const float* gt_cls, const float* gt_box, int n_gt, int nc, double conf,
                        double iou_thres, int* matrix, int* status, void* stream);
/* The drop-in's single image: gt_box (n_gt, 4) prepared xyxy fp32, gt_cls (n_gt) int32, det (n_det, 6) [x1, y1, x2, y2, conf, cls] fp32
 * or (det_f64) f64, or NULL (`detections=None`).  As above, except that an image without gts counts every detection above conf as
 * matrix[cls, nc] (utils/metrics.py:330-336). */
int y3d_confusion_image(const float* gt_box, const int* gt_cls, int n_gt, const void* det, int det_f64, int n_det, int nc, double conf,
                        double iou_thres, int* matrix, int* status, void* stream);
/* ap_per_class core: n detections sorted by (class, confidence descending); ucls (nc) int32 classes with targets, nl (nc) f64 = n_l + eps;
 * x_ap (n_ap <= 129) / x_curve (n_curve <= 1024) f64 ascending grids -> ap (nc, n_thr), p_curve / r_curve (nc, n_curve) f64 */
int y3d_ap_per_class(const int* tp, const double* conf, const int* cls, int64_t n, const int* ucls, const double* nl, int nc, int n_thr,
                     const double* x_ap, int n_ap, const double* x_curve, int n_curve, double* ap, double* p_curve, double* r_curve,
                     void* stream);

/* ------------------------------------------------------------------------------------------------
 * Optimizer step as multi-tensor launches (optim.hip): clip_grad_norm_ + SGD(nesterov, weight decay), AdamW, and the rest of the
 * reference's list (Adam, Adamax, NAdam, RAdam, RMSprop) — engine/trainer.py:567-575, 734-790.  All table arguments are DEVICE arrays: tensor t has sizes[t] fp32 elements at param_ptrs[t] / grad_ptrs[t] / buf_ptrs[t];
 * workgroup c handles elements [chunk_off[c]*chunk, +chunk) of tensor chunk_tensor[c].
 * ---------------------------------------------------------------------------------------------- */
int y3d_mt_sqnorm(const int64_t* grad_ptrs, const int64_t* sizes, const int* chunk_tensor, const int* chunk_off, int nchunks, int chunk,
                  float* partials, void* stream);
/* dst_t = src_t * scale for every tensor of the table (same table layout): the step's gradient tensors -> the flat buffer that is
 * all-reduced over RCCL (ddp.FlatGradReducer; reference: DistributedDataParallel's gradient buckets, engine/trainer.py:225-236) */
int y3d_mt_copy(const int64_t* src_ptrs, const int64_t* dst_ptrs, const int64_t* sizes, const int* chunk_tensor, const int* chunk_off,
                int nchunks, int chunk, float scale, void* stream);
/* acc_t += grad_t for every tensor of the table (same table layout), one fp32 add per element: a micro-batch's gradients into the
 * accumulation arena of optim.GradAccumulator (reference: the `accumulate` backward passes per optimizer step, engine/trainer.py:384-386,
 * 411-413, which autograd adds tensor by tensor) */
int y3d_mt_grad_acc(const int64_t* acc_ptrs, const int64_t* grad_ptrs, const int64_t* sizes, const int* chunk_tensor, const int* chunk_off,
                    int nchunks, int chunk, void* stream);
/* out[0] = total gradient L2 norm, out[1] = min(1, max_norm / (norm + 1e-6)) */
int y3d_mt_clip_coef(const float* partials, int nchunks, float max_norm, float* out_norm_clip, void* stream);
/* g = grad*clip (+ wd*p); buf = first ? g : momentum*buf + g; p -= lr * (nesterov ? g + momentum*buf : buf) */
int y3d_mt_sgd(const int64_t* param_ptrs, const int64_t* grad_ptrs, const int64_t* buf_ptrs, const int64_t* sizes, const float* lr,
               const float* wd, const int* chunk_tensor, const int* chunk_off, int nchunks, int chunk, float momentum, int nesterov,
               int first_step, const float* norm_clip, void* stream);

/* torch.optim.AdamW step (amsgrad off) — the reference's optimizer for short schedules (engine/trainer.py:752-764, `optimizer: auto`):
 * g = grad*clip; p *= 1 - lr*wd; m += (1-beta1)(g - m); v = beta2 v + (1-beta2) g^2; p -= lr/bias_corr1 * m / (sqrt(v)/bias_corr2_sqrt + eps) */
int y3d_mt_adamw(const int64_t* param_ptrs, const int64_t* grad_ptrs, const int64_t* m_ptrs, const int64_t* v_ptrs, const int64_t* sizes,
                 const float* lr, const float* wd, const int* chunk_tensor, const int* chunk_off, int nchunks, int chunk, float beta1, float beta2,
                 float eps, float bias_corr1, float bias_corr2_sqrt, const float* norm_clip, void* stream);
/* The reference's remaining optimizers (engine/trainer.py:776-781: Adam, Adamax, NAdam, RAdam, RMSProp) and a schedulable momentum.
 *
 * y3d_mt_step_scalars: one workgroup, after y3d_mt_clip_coef.  Reads the finite flag norm_clip[2] and the applied-step count
 * t = norm_clip[3] and writes, computed in double and rounded once to float, what the update kernels need that depends only on t
 * (betas as fp32 values, as the update kernels use them):
 *   [0] 1-beta1^t   [1] 1-beta2^t   [2] sqrt([0])   [3] sqrt([1])
 *   [4] mu_t = beta1 (1 - 0.5 0.96^(t momentum_decay))   [5] mu_{t+1}   [6] mu_product (fp32 STATE: *= mu_t, 1 before the first applied
 *   step)   [7] mu_product mu_{t+1}   [12] (1-mu_t)/(1-mu_product)   [13] mu_{t+1}/(1-[7])                      (torch.optim.NAdam)
 *   [8] rho_t = rho_inf - 2 t beta2^t/(1-beta2^t)   [9] rho_t > 5 (decided in double) ? 1 : 0   [10] the rectification factor
 *   sqrt((rho_t-4)(rho_t-2)rho_inf / ((rho_inf-4)(rho_inf-2)rho_t)) when [9], else 0                             (torch.optim.RAdam)
 *   [11] t   [14], [15] unused
 * A skipped step (norm_clip[2] == 0) leaves all Y3D_STEP_SCALARS floats as they are. */
#define Y3D_STEP_SCALARS 16
int y3d_mt_step_scalars(const float* norm_clip, float beta1, float beta2, double momentum_decay, float* step_scalars, void* stream);
/* One step of torch.optim.{Adam, Adamax, NAdam, RAdam, RMSprop} in torch's single-tensor arithmetic (foreach=False, amsgrad / centered /
 * maximize off, coupled weight decay g += wd*p), tables and skip rule as y3d_mt_sgd; norm_clip may be NULL (coefficient 1, no skip).
 * g = grad*clip (+ wd*p);  s0 / s1 are the two state buffers:
 *   ADAM    m += (1-beta1)(g-m); v = beta2 v + (1-beta2) g^2; p -= lr/[0] * m / (sqrt(v)/[3] + eps)
 *   ADAMAX  m as above; u = max(beta2 u, |g| + eps); p -= lr/[0] * m / u
 *   NADAM   m, v as ADAM; d = sqrt(v/[1]) + eps; p -= lr [12] * g/d; p -= lr [13] * m/d
 *   RADAM   m, v as ADAM; [9] ? p -= m/[0] * lr * ([3] / (sqrt(v) + eps)) * [10] : p -= m/[0] * lr
 *   RMSPROP s0 = beta2 s0 + (1-beta2) g^2 (beta2 = alpha); q = g / (sqrt(s0) + eps); momentum[t] > 0 ? (s1 = momentum[t] s1 + q;
 *           p -= lr s1) : p -= lr q.   beta1 and step_scalars are not read; `momentum` is a per-tensor device table like lr / wd
 * ([i]: step_scalars[i]; `momentum` is read by RMSPROP only and may be NULL otherwise) */
#define Y3D_OPT_ADAM 0
#define Y3D_OPT_ADAMAX 1
#define Y3D_OPT_NADAM 2
#define Y3D_OPT_RADAM 3
#define Y3D_OPT_RMSPROP 4
int y3d_mt_update(int kind, const int64_t* param_ptrs, const int64_t* grad_ptrs, const int64_t* s0_ptrs, const int64_t* s1_ptrs,
                  const int64_t* sizes, const float* lr, const float* wd, const float* momentum, const int* chunk_tensor, const int* chunk_off,
                  int nchunks, int chunk, float beta1, float beta2, float eps, const float* step_scalars, const float* norm_clip, void* stream);
/* y3d_mt_sgd with the momentum read from a per-tensor device table next to lr / wd, so that a captured step follows a momentum
 * schedule (the reference's warm-up, engine/trainer.py:392-393) through in-place writes of that table */
int y3d_mt_sgd_tab(const int64_t* param_ptrs, const int64_t* grad_ptrs, const int64_t* buf_ptrs, const int64_t* sizes, const float* lr,
                   const float* wd, const float* momentum, const int* chunk_tensor, const int* chunk_off, int nchunks, int chunk, int nesterov,
                   int first_step, const float* norm_clip, void* stream);
/* ModelEMA.update (utils/torch_utils.py:431-443, called from optimizer_step engine/trainer.py:574-575): e = e*decay + (1-decay)*m over
 * every floating-point state_dict tensor, reps[t] times for tensor t (the reference walks state_dict KEYS, and the aliased one-to-one
 * head branches appear under two keys each).  guard: NULL, or y3d_mt_clip_coef's array — the update is then a no-op when
 * guard[2] == 0 (it follows an optimizer step that was skipped) */
int y3d_mt_ema(const int64_t* ema_ptrs, const int64_t* model_ptrs, const int64_t* sizes, const int* reps, const int* chunk_tensor,
               const int* chunk_off, int nchunks, int chunk, float decay, float one_minus_decay, const float* guard, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Depth predictor of the 3D head (nn/modules/head.py:978-1042 DepthPredictor), group_norm.hip / resize.hip
 * ---------------------------------------------------------------------------------------------- */
/* nn.GroupNorm(32, 128) over a conv's raw output y (written WITHOUT the conv bias): x = y + bconv[c], xhat = (x - mean[b,g]) * rstd[b,g],
 * z = xhat * gamma[c] + beta[c]; out = act(scale * sum_{i < nsrc} z_i), nsrc 1 or 3 (head.py:1027: the three-branch average), relu 0 / 1.
 * Only C = 128, G = 32 is built.  y / ysw / bconv / gamma / beta / dy / dysw: HOST arrays of nsrc device pointers / pixel strides; every
 * map is B * HW pixels at its pixel stride (elements), 16-byte aligned.  A chunk is 256 pixels of one sample:
 *   y3d_gn_stats      partials [nsrc][B][y3d_gn_chunks(HW)][G][2] = (mean, M2) of every chunk, two passes over it
 *   y3d_gn_apply      folds them per sample in chunk order (Chan's merge) in its prologue, writes out and stats [nsrc][B][G][2] = (mean, rstd)
 *   y3d_gn_bwd_reduce partials [B][chunks][2 nsrc + 1][C] = per channel sum dzh xhat_i | sum xhat_i | sum dzh, dzh = dz * scale * mask (the
 *                     ReLU mask recomputed from y, bconv and stats)
 *   y3d_gn_bwd_apply  dy_i = rstd (dzh gamma - (s1 + xhat s2) / n) in `dtype`, and dgamma / dbeta / dbconv [nsrc][C] (fp32) folded over
 *                     samples and chunks in a fixed order.  No float atomics anywhere: the same bits on every run. */
int y3d_gn_chunks(int HW);
int y3d_gn_stats(int dtype, int nsrc, const void* const* y, const int64_t* ysw, const float* const* bconv, int B, int HW, int C, int G,
                 float* partials, void* stream);
int y3d_gn_apply(int dtype, int nsrc, const void* const* y, const int64_t* ysw, const float* const* bconv, const float* const* gamma,
                 const float* const* beta, const float* partials, float eps, float scale, int relu, void* out, int64_t osw, float* stats, int B,
                 int HW, int C, int G, void* stream);
int y3d_gn_bwd_reduce(int dtype, int nsrc, const void* const* y, const int64_t* ysw, const float* const* bconv, const float* const* gamma,
                      const float* const* beta, const float* stats, float scale, int relu, const void* dz, int64_t dsw, float* partials, int B,
                      int HW, int C, int G, void* stream);
int y3d_gn_bwd_apply(int dtype, int nsrc, const void* const* y, const int64_t* ysw, const float* const* bconv, const float* const* gamma,
                     const float* const* beta, const float* stats, float scale, int relu, const void* dz, int64_t dsw, const float* partials,
                     void* const* dy, const int64_t* dysw, float* dgamma, float* dbeta, float* dbconv, int B, int HW, int C, int G, void* stream);
/* F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=False) over an NHWC map and its adjoint (a gather in a fixed order, no
 * atomics); C % 8 == 0; y, dy and dx are pixel-dense at their pixel strides */
int y3d_resize_bilinear_fwd(int dtype, const void* x, int64_t xsb, int64_t xsh, int64_t xsw, void* y, int64_t ysw, int B, int H, int W, int Ho,
                            int Wo, int C, void* stream);
int y3d_resize_bilinear_bwd(int dtype, const void* dy, int64_t dsw, void* dx, int64_t xsw, int B, int H, int W, int Ho, int Wo, int C,
                            void* stream);
/* out[c] = sum over M pixels of x[p][c] (fp32), C <= 256 in whole 16-byte chunks: per-block partials [y3d_colsum_blocks(M)][C], then one
 * fold in block order (the depth classifier's bias gradient) */
int y3d_colsum_blocks(int64_t M);
int y3d_colsum(int dtype, const void* x, int64_t xsw, int64_t M, int C, float* partials, float* out, void* stream);
/* out[cell] = sum_c softmax(logits[cell])_c * bins[c] (head.py:1036-1037 weighted_depth), fp32, one thread per cell; the logits' rows
 * (pixel stride sw) hold the C channels in whole 16-byte chunks */
int y3d_depth_expect(int dtype, const void* logits, int64_t sw, int64_t M, int C, const float* bins, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* Y3D_H */
