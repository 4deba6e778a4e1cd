"""fp8 MFMA conv forward (csrc/conv3x3_fp8.hip) next to the bf16 persistent kernel on the head shapes, through the C ABI (HIP events,
back-to-back launches on random operands).  python tools/fp8_conv_bench.py [B] [--dgrad]
--dgrad: the data gradient of the same layers instead - bf16 conv2d_bwd_data against y3d_conv3x3_fp8_dgrad, the stand-alone gradient
quantiser over the channels the data gradient reads, and the BatchNorm-backward apply pass that produces dy (what a fused copy would have to beat)."""
import sys, torch
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import yolov10_3d_amd as y3d
from yolov10_3d_amd import ops
from test_hip_fp8 import quantize_act, pack_weight
DEV = "cuda"
_pos = [a for a in sys.argv[1:] if not a.startswith("--")]
B = int(_pos[0]) if _pos else 32
DGRAD = "--dgrad" in sys.argv
L = ops.lib()

def timeit(fn, n=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n



def dgrad_table():
    """per head / body layer (Cin -> Cout, its data gradient reads Cout channels of dy and writes Cin): bf16 vs fp8 data gradient, the gradient
    quantiser, and the apply pass.  FLOPs = 2 B H W Cout (Cin / g) 9; the yardstick is the bf16 call the switch-off path makes."""
    from test_hip_fp8_dgrad import quantize_weight, pack_dgrad, quantize_grad
    bf = ops.code(torch.bfloat16)
    print(f"{'layer (data gradient of)':44s} {'bf16 ms':>8s} {'TF/s':>6s} {'fp8 ms':>8s} {'TF/s':>6s} {'quant ms':>9s} {'apply':>7s}  speed-up conv only / "
          "with quantiser")
    for (Cin, Cout, g, H, W, lo) in [(2048, 2048, 16, 80, 80, 0), (128, 2048, 1, 80, 80, 1024), (2048, 2048, 16, 40, 40, 0), (256, 2048, 1, 40, 40, 1024),
                                     (2048, 2048, 16, 20, 20, 0), (512, 2048, 1, 20, 20, 1024), (128, 128, 1, 80, 80, 0), (128, 128, 1, 40, 40, 0)]:
        torch.manual_seed(0)
        P, co = B * H * W, Cout - lo
        dy = (torch.randn(B, Cout, H, W, device=DEV) * 1e-3).to(torch.bfloat16)
        dyn = ops.to_nhwc(dy, torch.bfloat16, dense=True)
        w = torch.randn(Cout, Cin // g, 3, 3, device=DEV) * 0.05
        flops = 2.0 * P * co * (Cin // g) * 9
        kp = L.conv_kpad(bf, 9 * (co // g))
        wpd = torch.empty(Cin * kp, dtype=torch.bfloat16, device=DEV)
        L.pack_weight_dgrad(bf, w.data_ptr() + lo * (Cin // g) * 9 * 4, wpd.data_ptr(), co, Cin // g, g, 3, 3, ops.stream())
        dx = ops.nhwc_empty(B, Cin, H, W, torch.bfloat16, DEV)
        dsb, dsh, dsw = ops.s3(dyn)
        t16 = timeit(lambda: L.conv2d_bwd_data(bf, dyn.data_ptr() + lo * 2, dsb, dsh, dsw, B, H, W, co, wpd.data_ptr(), dx.data_ptr(), dx.stride(3), H, W, Cin, g, 3, 3, 1, 1,
                                               ops.stream()))
        codes, scale, _ = quantize_weight(w)
        q, s = quantize_grad(dy, scale)
        wq, ws = pack_dgrad(codes, Cout, Cin, g, lo, Cout)
        t8 = timeit(lambda: L.conv3x3_fp8_dgrad(q.data_ptr(), s.data_ptr(), Cout, s.shape[3], lo, Cout, B, H, W, wq.data_ptr(), ws.data_ptr(), dx.data_ptr(), dx.stride(3), Cin, g,
                                                ops.stream()))
        # the stand-alone quantiser over the channels the data gradient reads (the window)
        qw = torch.empty(P, co, dtype=torch.uint8, device=DEV)
        sw_ = torch.empty(P, L.fp8_scale_pitch(co), dtype=torch.uint8, device=DEV)
        tq = timeit(lambda: L.fp8_quantize_grad(dyn.data_ptr() + lo * 2, Cout, scale.data_ptr() + lo * 4, P, co, qw.data_ptr(), sw_.data_ptr(), ops.stream()))
        # BatchNorm-backward apply over all Cout channels
        y = torch.randn(P, Cout, device=DEV).to(torch.bfloat16)
        st = [torch.rand(Cout, device=DEV) + 0.5 for _ in range(6)]
        dyo = torch.empty(P, Cout, dtype=torch.bfloat16, device=DEV)
        ta = timeit(lambda: L.bn_act_bwd_apply(bf, y.data_ptr(), Cout, dyn.data_ptr(), Cout, None, 0, st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(), st[3].data_ptr(),
                                               st[4].data_ptr(), st[5].data_ptr(), 1, 0, 1, dyo.data_ptr(), Cout, None, 0, P, Cout, ops.stream()))
        print(f"B={B} {Cin:4d}->{Cout} g={g:2d} @{H}x{W} dy[{lo}:{Cout}]".ljust(44) + f" {t16:8.3f} {flops / t16 / 1e9:6.0f} {t8:8.3f} {flops / t8 / 1e9:6.0f} {tq:9.3f} {ta:7.3f}"
              f"  x{t16 / t8:.2f} / x{t16 / (t8 + tq):.2f}")


def fwd_table():
    print(f"{'shape':44s} {'bf16 ms':>8s} {'TF/s':>6s} {'fp8 ms':>8s} {'TF/s':>6s} {'quant ms':>9s} speed-up (conv only / with quantiser)")
    for (Cin, Cout, g, H, W) in [(2048, 2048, 16, 80, 80), (128, 2048, 1, 80, 80), (2048, 2048, 16, 40, 40), (256, 2048, 1, 40, 40), (2048, 2048, 16, 20, 20), (512, 2048, 1, 20, 20),
                                 (640, 2048, 1, 40, 40), (640, 2048, 1, 20, 20)]:
        torch.manual_seed(0)
        x = torch.nn.functional.silu(torch.randn(B, Cin, H, W, device=DEV)).to(torch.bfloat16)
        xin = ops.to_nhwc(x, torch.bfloat16, dense=True)
        w = (torch.randn(Cout, Cin // g, 3, 3, device=DEV) * 0.05)
        flops = 2.0 * B * H * W * Cout * (Cin // g) * 9
        # bf16
        wp = torch.empty(Cout * 9 * (Cin // g), dtype=torch.bfloat16, device=DEV)
        L.pack_weight_fwd(ops.code(torch.bfloat16), w.data_ptr(), wp.data_ptr(), Cout, Cin // g, Cin // g, 3, 3, ops.stream())
        y = ops.nhwc_empty(B, Cout, H, W, torch.bfloat16, DEV)
        rows = L.conv2d_stat_rows(ops.code(torch.bfloat16), B, H, W, Cin, Cout, g, 3, 3, 1, 1)
        part = torch.empty(rows * Cout * 2, dtype=torch.float32, device=DEV)
        sb, sh, sw = ops.s3(xin)
        t16 = timeit(lambda: L.conv2d_fwd(ops.code(torch.bfloat16), xin.data_ptr(), sb, sh, sw, B, H, W, Cin, wp.data_ptr(), None, y.data_ptr(), Cout, H, W, Cout, g, 3, 3, 1, 1,
                                          part.data_ptr(), ops.stream()))
        # fp8
        q, s = quantize_act(x)
        wq, ws, _ = pack_weight(w)
        rows8 = L.conv3x3_fp8_stat_rows(B, H, W)
        part8 = torch.empty(rows8 * Cout * 2, dtype=torch.float32, device=DEV)
        t8 = timeit(lambda: L.conv3x3_fp8_fwd(q.data_ptr(), s.data_ptr(), B, H, W, Cin, wq.data_ptr(), ws.data_ptr(), y.data_ptr(), y.stride(3), Cout, g, part8.data_ptr(), None, None, 0,
                                              ops.stream()))
        tq = timeit(lambda: L.fp8_quantize_act(xin.data_ptr(), xin.stride(3), B * H * W, Cin, q.data_ptr(), s.data_ptr(), ops.stream()))
        print(f"B={B} {Cin:4d}->{Cout} g={g:2d} @{H}x{W}".ljust(44) + f" {t16:8.3f} {flops / t16 / 1e9:6.0f} {t8:8.3f} {flops / t8 / 1e9:6.0f} {tq:9.3f}  x{t16 / t8:.2f} / x{t16 / (t8 + tq):.2f}")


if __name__ == "__main__":
    dgrad_table() if DGRAD else fwd_table()
