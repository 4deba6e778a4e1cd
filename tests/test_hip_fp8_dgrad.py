"""GPU: the fp8 (MX e4m3) data gradient of the fp8 MFMA convolutions (csrc/conv3x3_fp8.hip: y3d_fp8_quantize_grad,
y3d_fp8_pack_weight_dgrad, y3d_conv3x3_fp8_dgrad; ops.set_fp8_dgrad).  Stated bounds:
    * packer, quantisers: bytes equal to the restatements (tests/fp8_dgrad_ref.py, oracle/restate.py mx_quantize_act);
    * data gradient on operands whose quantisation is exact: bit-exact against torch.nn.grad.conv2d_input in float64, rounded once to bf16;
    * on real operands: |dx - ref| <= 2 K 2^-24 mag + 2^-8 |ref| with K = 9 Cout / g against the float64 data gradient of the SAME quantised
      operands (the forward test's bound with the swapped depth);
    * through autograd and the whole model: switch off = the parent's path bit for bit; switch on = the kernel-level result bit for bit,
      weight gradients that no data gradient feeds unchanged, the rest within the caps of the forward's full-model test."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import yolov10_3d_amd as y3d  # noqa: E402
from yolov10_3d_amd import ops  # noqa: E402
from oracle import restate as RS  # noqa: E402  (the checker)
from fp8_dgrad_ref import e4m3_value, pack_dgrad_ref  # noqa: E402
from test_hip_fp8 import CONV_CASES  # noqa: E402

DEV = "cuda"
conv2d_input = torch.nn.grad.conv2d_input


def quantize_weight(w):
    """fp32 OIHW master (device) -> (codes (rows, K) uint8, scale (rows,) fp32, w_eff) through the fp8w quantiser"""
    w = w.float().contiguous()
    rows, K = w.shape[0], w[0].numel()
    codes = torch.empty(rows, K, dtype=torch.uint8, device=w.device)
    weff = torch.empty_like(w)
    scale = torch.empty(rows, dtype=torch.float32, device=w.device)
    desc = torch.tensor([w.data_ptr(), weff.data_ptr(), codes.data_ptr(), scale.data_ptr(), rows, K], dtype=torch.int64, device=w.device)
    rb = torch.zeros(1, dtype=torch.int32, device=w.device)
    ops.lib().mt_fp8w_quantize(desc.data_ptr(), rb.data_ptr(), 1, rows, ops.stream())
    return codes, scale, weff


def pack_dgrad(codes, Cout, Cin, g, lo, hi):
    wq = torch.full((g, Cin // g, 9, (hi - lo) // g), 0xAA, dtype=torch.uint8, device=codes.device)
    ws = torch.zeros(Cin, dtype=torch.uint8, device=codes.device)
    ops.lib().fp8_pack_weight_dgrad(codes.data_ptr(), Cout, Cin, g, lo, hi, wq.data_ptr(), ws.data_ptr(), ops.stream())
    return wq, ws


def quantize_grad(dy, scale):
    """bf16 (B, C, H, W) device, scale (C,) fp32 -> (codes (B, H, W, C), scales (B, H, W, pitch)) through y3d_fp8_quantize_grad"""
    d = ops.to_nhwc(dy, torch.bfloat16, dense=True)
    B, C, H, W = d.shape
    q = torch.empty(B, H, W, C, dtype=torch.uint8, device=d.device)
    s = torch.zeros(B, H, W, ops.lib().fp8_scale_pitch(C), dtype=torch.uint8, device=d.device)
    ops.lib().fp8_quantize_grad(d.data_ptr(), d.stride(3), scale.data_ptr(), B * H * W, C, q.data_ptr(), s.data_ptr(), ops.stream())
    return q, s


def dgrad_fp8(dy, w, Cin, g, lo=0, hi=None, dx=None):
    """the kernel-level data gradient: dy (B, Cout, H, W) bf16 on the device (all Cout channels), w the fp32 master -> dx bf16"""
    B, Cout, H, W = dy.shape
    hi = Cout if hi is None else hi
    codes, scale, _ = quantize_weight(w)
    q, s = quantize_grad(dy, scale)
    wq, ws = pack_dgrad(codes, Cout, Cin, g, lo, hi)
    if dx is None:
        dx = ops.nhwc_empty(B, Cin, H, W, torch.bfloat16, dy.device)
    ops.lib().conv3x3_fp8_dgrad(q.data_ptr(), s.data_ptr(), Cout, s.shape[3], lo, hi, B, H, W, wq.data_ptr(), ws.data_ptr(), dx.data_ptr(), dx.stride(3), Cin, g,
                                ops.stream())
    torch.cuda.synchronize()
    return dx


# ---- 4. the packer ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(128, 256, 1, 0, 256), (96, 128, 2, 0, 128), (2048, 2048, 16, 0, 2048), (128, 1024, 1, 256, 768)],
                         ids=["g1", "g2", "g16", "window"])
def test_fp8_dgrad_weight_packer_bytes_equal_the_restatement(case):
    Cin, Cout, g, lo, hi = case
    torch.manual_seed(Cin + Cout)
    codes = torch.randint(0, 256, (Cout, Cin // g, 3, 3), dtype=torch.uint8)
    wq, ws = pack_dgrad(codes.to(DEV).reshape(Cout, -1).contiguous(), Cout, Cin, g, lo, hi)
    torch.cuda.synchronize()
    assert torch.equal(wq.cpu(), torch.from_numpy(pack_dgrad_ref(codes.numpy(), g, lo, hi)))
    assert torch.equal(ws.cpu(), torch.full((Cin,), 127, dtype=torch.uint8)), "unit E8M0 row scales"


# ---- 5. the quantisers -----------------------------------------------------------------------------------------------------------------
def _grad_like(shape, seed):
    torch.manual_seed(seed)
    B, C, H, W = shape
    dy = torch.randn(B, C, H, W) * torch.exp2(torch.randint(-24, -4, (B, C // 32, 1, H, W)).float()).repeat_interleave(32, 1).reshape(B, C, H, W)
    dy[0, :32, 0, 0] = 0.0                   # an all-zero block: scale byte 127
    dy[0, 32:64, 0, 1] = 1e-7                # gradient-like magnitudes
    dy = dy.to(torch.bfloat16)
    scale = torch.exp2(torch.randint(-14, 3, (C,)).float())
    return dy, scale


@pytest.mark.parametrize("shape", [(2, 64, 5, 7), (1, 128, 16, 16), (3, 96, 3, 9)])
def test_fp8_grad_quantizer_bit_exact_vs_oracle(shape):
    B, C, H, W = shape
    dy, scale = _grad_like(shape, sum(shape))
    assert float(dy.float().abs()[dy != 0].min()) < 1e-7
    q, s = quantize_grad(dy.to(DEV), scale.to(DEV))
    torch.cuda.synchronize()
    cq, cs, _ = RS.mx_quantize_act(dy.float() * scale.view(1, -1, 1, 1))
    assert torch.equal(s.cpu()[..., : C // 32].permute(0, 3, 1, 2), cs), "E8M0 scale bytes differ"
    assert torch.equal(q.cpu().permute(0, 3, 1, 2), cq), "e4m3 codes differ"
    assert int(cs[0, 0, 0, 0]) == 127


# ---- 6. exact on integer operands --------------------------------------------------------------------------------------------------------
EXTRA = [  # B, Cin, Cout, groups, H, W, lo, hi (None: all), dx channel offset in a wider buffer (None: own tensor)
    (3, 128, 128, 1, 4, 8, 0, None, None), (3, 128, 128, 1, 5, 9, 0, None, None), (2, 128, 128, 1, 9, 23, 0, None, None),
    (5, 128, 128, 1, 20, 20, 0, None, None), (1, 128, 128, 1, 80, 80, 0, None, None),
    (1, 256, 2048, 1, 8, 16, 0, None, None), (1, 512, 2048, 1, 8, 8, 0, None, None),
    (2, 128, 1024, 1, 12, 16, 256, 768, None), (3, 128, 256, 1, 8, 16, 0, None, 64), (2, 64, 512, 1, 8, 16, 256, 512, 32),
]
INT_CASES = [c + (0, None, None) for c in CONV_CASES] + EXTRA


def _int_operands(B, Cin, Cout, g, H, W):
    torch.manual_seed(Cin + Cout + H)
    dy = torch.randint(-3, 4, (B, Cout, H, W)).float() * (torch.rand(B, Cout, H, W) < 0.3)
    dy = dy * torch.exp2(torch.randint(-3, 4, (B, Cout // 32, 1, H, W)).float()).repeat_interleave(32, 1).reshape(B, Cout, H, W)
    w = torch.randint(-2, 3, (Cout, Cin // g, 3, 3)).float() * (torch.rand(Cout, Cin // g, 3, 3) < 0.25)
    w = w * torch.exp2(torch.randint(-4, 3, (Cout, 1, 1, 1)).float())
    return dy, w


@pytest.mark.parametrize("case", INT_CASES, ids=[str(c) for c in INT_CASES])
def test_fp8_dgrad_exact_on_integer_operands(case):
    """dy in {0, +-1, +-2, +-3} x a per-block power of two, weights in {0, +-1, +-2} x a per-row power of two: the folded dy quantises
    exactly (checked), every product and fp32 partial sum is exact, so dx must equal conv2d_input in float64 rounded once to bf16.  A
    geometry the kernel does not serve must be refused by _ok AND by the launcher (an error, no fallback in the C layer)."""
    B, Cin, Cout, g, H, W, lo, hi, slot = case
    hi = Cout if hi is None else hi
    L = ops.lib()
    dy, w = _int_operands(B, Cin, Cout, g, H, W)
    if not L.conv3x3_fp8_dgrad_ok(B, H, W, Cin, hi - lo, g):
        assert (Cout // g) % 64 or Cout // g < 128 or (Cin // g) % 16
        with pytest.raises(y3d.Y3DError, match="not served"):
            dgrad_fp8(dy.to(torch.bfloat16).to(DEV), w.to(DEV), Cin, g, lo, hi)
        return
    codes, scale, w_eff = RS.fp8w_quantize(w)
    assert torch.equal(w_eff, w), "precondition: the weights are fp8w-exact"
    folded = dy * scale.view(1, -1, 1, 1)
    assert torch.equal(RS.mx_quantize_act(folded)[2], folded), "precondition: the folded dy is MX-exact"
    ref = conv2d_input((B, Cin, H, W), w[lo:hi].double(), dy[:, lo:hi].double(), 1, 1, 1, g)
    assert float(ref.abs().max()) < 2 ** 15
    refb = ref.float().to(torch.bfloat16).float()
    dx = None
    if slot is not None:
        buf = torch.full((B, H, W, Cin + 2 * slot), 7.5, dtype=torch.bfloat16, device=DEV).permute(0, 3, 1, 2)
        dx = buf[:, slot:slot + Cin]
    out = dgrad_fp8(dy.to(torch.bfloat16).to(DEV), w.to(DEV), Cin, g, lo, hi, dx)
    assert torch.equal(out.float().cpu(), refb), f"max |diff| {float((out.float().cpu() - refb).abs().max())}"
    if slot is not None:
        rest = torch.cat([buf[:, :slot], buf[:, slot + Cin:]], 1)
        assert bool((rest == 7.5).all()), "bytes outside the channel slice changed"


def test_fp8_dgrad_launcher_refuses_what_it_cannot_serve():
    L = ops.lib()
    assert not L.conv3x3_fp8_dgrad_ok(2, 3, 8, 128, 128, 1) and not L.conv3x3_fp8_dgrad_ok(2, 4, 7, 128, 128, 1)
    dy, w = _int_operands(2, 128, 256, 1, 8, 16)
    d, wd = dy.to(torch.bfloat16).to(DEV), w.to(DEV)
    with pytest.raises(y3d.Y3DError, match="multiple of 128"):
        dgrad_fp8(d, wd, 128, 1, 64, 256)            # window not on a 128-channel boundary
    with pytest.raises(y3d.Y3DError, match="not served"):
        dgrad_fp8(d[:, :, :3], wd, 128, 1)            # H = 3
    with pytest.raises(y3d.Y3DError, match="not served"):
        dgrad_fp8(d[:, :, :, :7], wd, 128, 1)         # W = 7
    dx = ops.nhwc_empty(2, 136, 8, 16, torch.bfloat16, DEV)[:, 4:132]
    with pytest.raises(y3d.Y3DError, match="dx pixel stride"):
        dgrad_fp8(d, wd, 128, 1, dx=dx)               # rows of dx not 16-byte aligned


# ---- 7. real operands --------------------------------------------------------------------------------------------------------------------
REAL_CASES = [(4, 128, 256, 1, 16, 16, 0, None), (2, 2048, 2048, 16, 20, 20, 0, None), (2, 256, 2048, 1, 12, 16, 1024, 2048)]


def _real_operands(B, Cin, Cout, g, H, W):
    torch.manual_seed(7)
    dy = (torch.randn(B, Cout, H, W) * torch.exp(torch.randn(B, 1, H, W) * 1.5) * 1e-4).to(torch.bfloat16)  # heavy-tailed: Gaussian x log-normal per pixel
    w = torch.randn(Cout, Cin // g, 3, 3) * 0.05 * torch.exp2(torch.randint(-3, 2, (Cout, 1, 1, 1)).float())
    return dy, w


@pytest.mark.parametrize("case", REAL_CASES, ids=["128to256", "head_layer2_p5", "head_layer1_window"])
def test_fp8_dgrad_real_operands_within_accumulation_bound(case):
    B, Cin, Cout, g, H, W, lo, hi = case
    hi = Cout if hi is None else hi
    dy, w = _real_operands(B, Cin, Cout, g, H, W)
    dx = dgrad_fp8(dy.to(DEV), w.to(DEV), Cin, g, lo, hi)
    codes, scale, w_eff = RS.fp8w_quantize(w)
    val = e4m3_value(codes.numpy()).reshape(w.shape)
    dy_eff = RS.mx_quantize_act(dy.float() * scale.view(1, -1, 1, 1))[2].double()
    ref = conv2d_input((B, Cin, H, W), val[lo:hi], dy_eff[:, lo:hi], 1, 1, 1, g)
    mag = conv2d_input((B, Cin, H, W), val[lo:hi].abs(), dy_eff[:, lo:hi].abs(), 1, 1, 1, g)
    K = 9 * (hi - lo) // g
    bound = 2 * K * 2.0 ** -24 * mag + 2.0 ** -8 * ref.abs() + 1e-30
    err = (dx.double().cpu() - ref).abs()
    assert bool((err <= bound).all()), f"worst error / bound {float((err / bound).max()):.3f}"
    # the format itself (a property of the emulation, reported only): against the unquantised float64 data gradient of (dy, w_eff)
    full = conv2d_input((B, Cin, H, W), w_eff[lo:hi].double(), dy[:, lo:hi].double(), 1, 1, 1, g)
    print(f"fp8 data gradient {case}: worst error / bound {float((err / bound).max()):.3f}; format cost (MX dy vs bf16 dy, same weights) relative L2 "
          f"{float((ref - full).norm() / full.norm()):.3e}")


# ---- 8. autograd, one layer ----------------------------------------------------------------------------------------------------------------
def _layer_step(m, x0, up, dgrad_on):
    """one forward + backward of Conv module m with fp8 weights + fp8 forward; -> (dx, dW, dgamma, dbeta, timer keys, recorded dy)"""
    rec = {}
    inner = ops._conv_backward

    def spy(cfg, saved, dy, *a, **k):
        rec["dy"] = dy.clone()
        return inner(cfg, saved, dy, *a, **k)

    y3d.set_fp8_dgrad(dgrad_on)
    m.zero_grad(set_to_none=True)
    x = x0.clone().requires_grad_(True)
    seen = []
    ops.TIMER = ops.KernelTimer(lambda key: seen.append(key[0]) or False)
    ops._conv_backward = spy
    try:
        z = m(x)
        (z.float() * up).sum().backward()
    finally:
        ops._conv_backward = inner
        ops.TIMER = None
    torch.cuda.synchronize()
    return x.grad.clone(), m.conv.weight.grad.clone(), m.bn.weight.grad.clone(), m.bn.bias.grad.clone(), seen, rec["dy"]


@pytest.mark.parametrize("case", [(3, 128, 128, 12, 20, True), (2, 128, 256, 8, 16, True), (3, 96, 96, 12, 20, False), (2, 128, 128, 3, 8, False)],
                         ids=["128to128", "128to256", "96to96_not_served", "3x8_map_not_served"])
def test_fp8_dgrad_through_autograd_one_layer(case):
    from yolov10_3d_amd import modules as M
    B, Cin, Cout, H, W, served = case
    torch.manual_seed(Cin + H)
    y3d.set_compute_dtype(torch.bfloat16)
    y3d.set_weight_quant("fp8")
    try:
        y3d.set_fp8_conv(True)
        m = M.Conv(Cin, Cout, 3).to(DEV).train()
        m.bn.weight.data.uniform_(0.5, 1.5)
        x0 = torch.nn.functional.silu(torch.randn(B, Cin, H, W)).to(torch.bfloat16).to(DEV)
        up = (torch.randn(B, Cout, H, W) * torch.exp(torch.randn(B, 1, H, W)) * 1e-3).to(DEV)
        off = _layer_step(m, x0, up, False)
        on = _layer_step(m, x0, up, True)
        on2 = _layer_step(m, x0, up, True)
        for r in (on, on2):
            assert torch.equal(r[1], off[1]) and torch.equal(r[2], off[2]) and torch.equal(r[3], off[3]), "dW / dgamma / dbeta depend on no data gradient"
            assert torch.equal(r[5], off[5]), "dy (bf16) is the same tensor on every path"
        assert off[4].count("conv_dgrad") == 1 and off[4].count("conv_dgrad_fp8") == 0
        if not served:
            for r in (on, on2):
                assert torch.equal(r[0], off[0]) and r[4].count("conv_dgrad_fp8") == 0 and r[4].count("conv_dgrad") == 1
            return
        for r in (on, on2):
            assert r[4].count("conv_dgrad_fp8") == 1 and r[4].count("conv_dgrad") == 0 and r[4].count("conv_fwd_fp8") == 1
        assert torch.equal(on[0], on2[0]), "two backward passes on the same inputs differ"
        want = dgrad_fp8(off[5], m.conv.weight.detach(), Cin, 1)
        assert torch.equal(on[0].float(), want.float()), "autograd's dx is not the kernel-level data gradient"
        assert not torch.equal(on[0], off[0]), "the bf16 data gradient came back: the test would not see the switch"
    finally:
        y3d.set_fp8_conv(False)
        y3d.set_weight_quant(None)
    assert ops.fp8_dgrad() is False


# ---- 9. / 10. whole model ------------------------------------------------------------------------------------------------------------------
def _head_params_no_dgrad_feeds(model):
    """ids of the head's layer-2 conv weights and projection weights / biases: their gradients come from the loss through BatchNorm and
    the projections only, no convolution data gradient lies upstream of them"""
    hd = model.model[-1]
    ids = set()
    for heads in (hd.o2o_heads, hd.o2m_heads):
        for h in heads:
            for lvl in h:
                ids |= {id(lvl[1].conv.weight), id(lvl[2].weight), id(lvl[2].bias)}
    return ids


def _model_step(model, state, batch, on):
    y3d.set_fp8_dgrad(on)
    model.load_state_dict(state)
    model.zero_grad(set_to_none=True)
    seen = []
    ops.TIMER = ops.KernelTimer(lambda key: seen.append(key) or False)
    try:
        loss, items = model.train()(batch)
        loss.backward()
    finally:
        ops.TIMER = None
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    return loss.detach().clone(), items.detach().clone(), grads, seen


def test_fp8_dgrad_full_model_step():
    """S-3D at 320x320, B = 4, fp8 weights + fp8 forward, data-gradient switch off vs on from the same state"""
    import bench
    torch.manual_seed(0)
    y3d.set_compute_dtype(torch.bfloat16)
    y3d.set_weight_quant("fp8")
    try:
        y3d.set_fp8_conv(True)
        model = y3d.YOLOv10_3DDetectionModel("yolov10s_3D.yaml").to(DEV).train()
        state = {k: v.clone() for k, v in model.state_dict().items()}
        batch = bench.synth_batch(4, 320, 320, 3, DEV)
        off = _model_step(model, state, batch, False)
        on = _model_step(model, state, batch, True)
        on2 = _model_step(model, state, batch, True)
    finally:
        y3d.set_fp8_conv(False)
        y3d.set_weight_quant(None)
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1]), "the forward is unchanged: loss and loss items are equal"
    launches = [k for k in on[3] if k[0] == "conv_dgrad_fp8"]
    print(f"conv_dgrad_fp8 launches: {len(launches)} (B, H, W, Cin, Cout, groups): {sorted({(k[2], k[3], k[4], k[5], k[6], k[9]) for k in launches})}; "
          f"bf16 conv_dgrad launches left: {sum(k[0] == 'conv_dgrad' for k in on[3])} of {sum(k[0] == 'conv_dgrad' for k in off[3])}")
    assert len(launches) > 0 and not any(k[0] == "conv_dgrad_fp8" for k in off[3])
    assert sum(k[0] == "conv_fwd_fp8" for k in on[3]) == sum(k[0] == "conv_fwd_fp8" for k in off[3])
    fixed = _head_params_no_dgrad_feeds(model)
    named = dict(model.named_parameters())
    nfix = 0
    for k, gr in off[2].items():
        if id(named[k]) in fixed:
            nfix += 1
            assert torch.equal(on[2][k], gr), f"{k}: no fp8 data gradient feeds this parameter, its gradient must not move"
    assert nfix >= 3 * 16 * 3
    # determinism: two eager steps from the same state
    for k, gr in on[2].items():
        assert torch.equal(on2[2][k], gr), f"{k}: two steps from the same state differ"
    rest = [k for k in off[2] if id(named[k]) not in fixed]
    norms = {k: float(off[2][k].float().norm()) for k in rest}
    floor = 1e-3 * max(norms.values())
    dev = sorted(abs(float(on[2][k].float().norm()) - v) / (v + floor) for k, v in norms.items())
    print(f"fp8 data gradient vs bf16 data gradient (S-3D 320^2 B=4, fp8 weights + fp8 forward): gradient norms of {len(rest)} parameters: median "
          f"{dev[len(dev) // 2]:.4f}, 90th percentile {dev[int(0.9 * len(dev))]:.4f}, max {dev[-1]:.4f}")
    assert any(not torch.equal(on[2][k], off[2][k]) for k in rest)
    assert dev[len(dev) // 2] < 0.05 and dev[int(0.9 * len(dev))] < 0.3


def test_fp8_dgrad_graphed_train_step_matches_eager_steps():
    """graph.GraphedTrainStep with the switch on: three replays leave the model where three eager steps leave it, bit for bit (the
    quantiser, the packer and the launcher neither allocate nor synchronise; the tables a capture bakes in are pinned)"""
    from bench import synth_batch
    from yolov10_3d_amd.graph import GraphedTrainStep
    from yolov10_3d_amd.optim import build_optimizer
    y3d.set_compute_dtype(torch.bfloat16)
    batches = [synth_batch(2, 256, 256, 20 + j, DEV) for j in range(3)]
    res = {}
    y3d.set_weight_quant("fp8")
    try:
        y3d.set_fp8_conv(True)
        y3d.set_fp8_dgrad(True)
        for mode in ("eager", "graph"):
            torch.manual_seed(3)
            model = y3d.YOLOv10_3DDetectionModel("yolov10s_3D.yaml").to(DEV).train()
            opt = build_optimizer(model, lr=0.01)
            model.model[-1].restack()
            items, n8 = [], 0
            if mode == "eager":
                for b in batches:
                    seen = []
                    ops.TIMER = ops.KernelTimer(lambda key: seen.append(key[0]) or False)
                    loss, it = model(b)
                    loss.backward()
                    ops.TIMER = None
                    n8 += seen.count("conv_dgrad_fp8")
                    opt.step(max_norm=10.0)
                    opt.zero_grad()
                    items.append(it.float().cpu())
                assert n8 >= 3, "the eager steps never launched the fp8 data gradient"
            else:
                step = GraphedTrainStep(model, opt, batches[0])
                for b in batches:
                    loss, it = step(b)
                    items.append(it.float().cpu().clone())
            torch.cuda.synchronize()
            res[mode] = (items, {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()}, opt.state.flat.cpu().clone())
    finally:
        ops.TIMER = None
        y3d.set_fp8_conv(False)
        y3d.set_weight_quant(None)
    for a, b in zip(res["eager"][0], res["graph"][0]):
        assert torch.equal(a, b), (a, b)
    for k, v in res["eager"][1].items():
        assert torch.equal(v, res["graph"][1][k]), f"state {k} differs after three steps"
    assert torch.equal(res["eager"][2], res["graph"][2]), "momentum buffers differ"
