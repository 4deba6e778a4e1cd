"""The zero-skip of csrc/proj_bn_mfma.hip (y3d_proj_group_bn_bwd mode 0, y3d_proj_group_bwd_weight_bn_mfma; switch
y3d_set_proj_zero_skip): pixel chunks whose `dout` rows of a branch are all +0 skip that branch's work.  Mode 1 (apply) runs the
dense path in both switch positions (its zero path measured slower: csrc/proj_bn_mfma.hip header) and is compared all the same.

Three branches with cout = (3, 24, 1) on cin = 128 and 64, bf16, act 0 and 1, the "strided" layout of proj_attn_ref.group_layout (odd
dsw, `dout` at an odd column).  P = 200: one 64-pixel step per BatchNorm run, a ragged last run (8 pixels), two 128-pixel steps in the
one weight-gradient run.  P = 8391: 128 BatchNorm runs of 128 pixels (two steps), runs 66.. wholly past the end; nine weight-gradient
runs of 1024 pixels (eight steps).

* ON EQUALS OFF: every output buffer (guard rows and uncovered columns included) is compared bit by bit between the two switch
  positions.  The off position is the dense path tests/test_hip_head_proj.py checks against float64.  mean_g is non-zero, so mode 1
  is bit-identical too; where a branch's mean_g is set to 0 (pattern "branch_zero") a stored zero may differ in sign and mode 1 is
  compared as numbers.
* AGAINST THE HOST: integer operands (exact sums, see tests/test_hip_head_proj.py) with sparse dout rows, switch on.
* THE SKIP HAPPENS: NaN in y wherever a branch's 32-pixel chunk has no dout (both of its 16-pixel chunks are then inactive as well):
  with the switch on, the mode-0 partials, slabs, dW and db are the bits of the run with finite y; with it off, 0 * NaN reaches them.
  (A run whose first 64 pixels are active in all four chunks is taken dense as a whole - the scan stops there so that a dense
  branch does not pay for it; the test leaves such runs finite.)"""
import ctypes

import pytest
import torch

import yolov10_3d_amd as y3d
from yolov10_3d_amd import ops
from yolov10_3d_amd._lib import BF16

import proj_attn_ref as R
from test_hip_attention import assert_exact, flat_slot, in_rows, out_slot

DEV = "cuda"
COUTS = (3, 24, 1)
TOT = sum(COUTS)
OOFF = (0, 3, 27)
SHAPES = [(200, 128), (200, 64), (8391, 128), (8391, 64)]


def IA(v):
    return (ctypes.c_int * len(v))(*v)


def PV(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class Rig:
    """operands of one (P, cin, act) on the device; run(skip) -> every output buffer of the three kernels"""

    def __init__(self, P, cin, act, y, dout, ws, scale, shift, mean, invstd, mg, mgx):
        self.P, self.cin, self.act = P, cin, act
        lay = R.group_layout(3, cin, COUTS, "strided", BF16, False)
        self.C, self.ysw, self.dsw, self.dysw, self.xoff = lay["C"], lay["xsw"], lay["dsw"], lay["dysw"], lay["xoff"]
        self.yd = in_rows(y, self.ysw, 8, torch.bfloat16)
        self.dd = in_rows(dout, self.dsw, 1, torch.bfloat16)
        self.wd = [w.float().to(DEV).contiguous() for w in ws]
        self.vec = [t.float().to(DEV) for t in (scale, shift, mean, invstd, mg, mgx)]
        L = y3d.lib()
        self.nrun, self.nblk = L.proj_group_bn_bwd_blocks(P), L.proj_group_bwd_weight_bn_mfma_blocks(P)
        self.ppb = -(-(-(-P // self.nrun)) // 64) * 64
        self.wpb = -(-(-(-P // self.nblk)) // 128) * 128

    def run(self, skip):
        L, st = y3d.lib(), ops.stream()
        P, cin, C = self.P, self.cin, self.C
        sc, sh, me, isd, mg, mgx = self.vec
        out = {}
        out["part"], part = out_slot(self.nrun, 2 * C, 2 * C, 0, torch.float32)
        out["dy"], dy = out_slot(P, C, self.dysw, 8, torch.bfloat16)
        out["slab"], slab = flat_slot(self.nblk * TOT * cin)
        out["bslab"], bslab = flat_slot(self.nblk * TOT)
        dws, dbs = [flat_slot(co * cin) for co in COUTS], [flat_slot(co) for co in COUTS]
        for br in range(3):
            out[f"dw{br}"], out[f"db{br}"] = dws[br][0], dbs[br][0]
        self.views = {"part": part, "dy": dy, "dw": [v for _, v in dws], "db": [v for _, v in dbs], "slab": slab}
        common = (3, cin, self.yd.data_ptr(), self.ysw, IA(self.xoff), self.dd.data_ptr(), self.dsw, PV(self.wd), IA(COUTS), sc.data_ptr(),
                  sh.data_ptr(), me.data_ptr(), isd.data_ptr())
        old = L.set_proj_zero_skip(skip)
        try:
            L.proj_group_bn_bwd(0, *common, None, None, self.act, part.data_ptr(), self.nrun, None, 0, P, C, st)
            L.proj_group_bn_bwd(1, *common, mg.data_ptr(), mgx.data_ptr(), self.act, None, 0, dy.data_ptr(), self.dysw, P, C, st)
            L.proj_group_bwd_weight_bn_mfma(3, cin, self.yd.data_ptr(), self.ysw, IA(self.xoff), self.dd.data_ptr(), self.dsw, IA(COUTS),
                                            sc.data_ptr(), sh.data_ptr(), self.act, slab.data_ptr(), bslab.data_ptr(),
                                            PV(self.views["dw"]), PV(self.views["db"]), P, st)
        finally:
            L.set_proj_zero_skip(old)
        return out


def real_rig(P, cin, act, dout=None):
    g = torch.Generator().manual_seed(P + cin + act)
    C = R.group_layout(3, cin, COUTS, "strided", BF16, False)["C"]
    y = (torch.randn(P, C, generator=g) * 2 + 0.5).bfloat16().double()
    ws = [(torch.randn(co, cin, generator=g) * 0.3) for co in COUTS]
    mean, invstd = y.mean(0), 1 / torch.sqrt(y.var(0, unbiased=False) + 1e-3)
    scale = (torch.rand(C, generator=g) + 0.5).double() * invstd
    shift = torch.randn(C, generator=g).double() - mean * scale
    mg, mgx = torch.randn(C, generator=g) * 0.1 + 0.5, torch.randn(C, generator=g) * 0.1
    assert bool((mg.float() != 0).all())
    return Rig(P, cin, act, y, torch.zeros(P, TOT) if dout is None else dout, ws, scale, shift, mean, invstd, mg, mgx), g


def same_bits(on, off, what, numeric=()):
    for k in on:
        if k in numeric:
            ok = bool(((on[k] == off[k]) | (on[k].isnan() & off[k].isnan())).all())
        else:
            ok = torch.equal(bits(on[k]), bits(off[k]))
        assert ok, f"{what}: `{k}` differs between zero-skip on and off ({int((bits(on[k]) != bits(off[k])).sum())} elements)"


def written(buf):
    """the elements a kernel stored (the sentinel is a NaN with a payload no kernel produces)"""
    return buf[~R.untouched(buf)]


def sparse_rows(P, density, g, ints=False):
    rows = torch.rand(P, generator=g) < density
    rows[torch.randint(0, P, (1,), generator=g)] = True
    vals = R.ints((P, TOT), 4, g) if ints else torch.randn(P, TOT, generator=g).bfloat16().double()
    return torch.where(rows[:, None], vals, torch.zeros_like(vals)), rows   # +0 elsewhere: vals * False would leave -0


@pytest.mark.gpu
def test_switch_returns_previous_value_and_restores():
    L = y3d.lib()
    first = L.set_proj_zero_skip(0)
    try:
        assert first == 1, "zero-skip is on by default"
        assert L.set_proj_zero_skip(1) == 0
        assert L.set_proj_zero_skip(7) == 1      # any non-zero value enables
        assert L.set_proj_zero_skip(0) == 1
        assert L.set_proj_zero_skip(0) == 0
    finally:
        L.set_proj_zero_skip(first)
    assert L.set_proj_zero_skip(first) == first


@pytest.mark.gpu
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("P,cin", SHAPES)
def test_on_equals_off_patterns(P, cin, act):
    rig, g = real_rig(P, cin, act)
    dd = rig.dd
    # 3: random rows at 2 % density; 4: dense; 5: -0 entries in otherwise zero rows (and a few rows that hold nothing else)
    sp, _ = sparse_rows(P, 0.02, g)
    dense = torch.randn(P, TOT, generator=g).bfloat16().double()
    for name, host in (("rows_2pct", sp), ("dense", dense)):
        dd.copy_(host.to(torch.bfloat16))
        same_bits(rig.run(1), rig.run(0), f"{name} P={P} cin={cin} act={act}")
    neg = torch.zeros(P, TOT, dtype=torch.int16)
    neg[torch.rand(P, TOT, generator=g) < 0.01] = -32768   # 0x8000
    neg[P - 1, TOT - 1] = -32768
    mixed = sp.to(torch.bfloat16).view(torch.int16).clone()
    mixed[mixed == 0] = neg[mixed == 0]
    for name, raw in (("neg_zero_only", neg), ("neg_zero_in_sparse_rows", mixed)):
        dd.copy_(raw.view(torch.bfloat16))
        assert bool((bits(dd) == -32768).any())
        same_bits(rig.run(1), rig.run(0), f"{name} P={P} cin={cin} act={act}")
    # 1: one branch all zero, the others dense; its mean_g = 0 on half of its channels: the stored zeros there may differ in sign
    for br in range(3):
        host = dense.clone()
        host[:, OOFF[br]:OOFF[br] + COUTS[br]] = 0
        dd.copy_(host.to(torch.bfloat16))
        mg = rig.vec[4].clone()
        rig.vec[4][rig.xoff[br]:rig.xoff[br] + cin:2] = 0
        same_bits(rig.run(1), rig.run(0), f"branch_zero[{br}] P={P} cin={cin} act={act}", numeric=("dy",))
        rig.vec[4].copy_(mg)


@pytest.mark.gpu
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("P,cin", SHAPES)
def test_on_equals_off_single_element(P, cin, act):
    """2: a single non-zero element: the edges of a 16-pixel chunk, a 32-pixel chunk, a 64- and a 128-pixel step, of a BatchNorm run
    and of a weight-gradient run, in the first and the last output of every branch"""
    rig, g = real_rig(P, cin, act)
    px = {0, 15, 16, 31, 32, 63, 64, P - 1}
    for run in {0, 1, (P - 1) // rig.ppb}:
        px |= {run * rig.ppb, min(P, (run + 1) * rig.ppb) - 1}
    for run in {0, (P - 1) // rig.wpb // 2, (P - 1) // rig.wpb}:
        px |= {run * rig.wpb, min(P, (run + 1) * rig.wpb) - 1}
    cols = sorted({OOFF[br] + o for br in range(3) for o in (0, COUTS[br] - 1)})
    rig.dd.zero_()
    zero_off = rig.run(0)
    for p in sorted(px):
        assert 0 <= p < P
        for i, c in enumerate(cols):
            rig.dd[p, c] = (-1.5, 0.75, 2.0)[(p + i) % 3]
            same_bits(rig.run(1), rig.run(0), f"single element at pixel {p} column {c}, P={P} cin={cin} act={act}")
            rig.dd[p, c] = 0
    same_bits(rig.run(1), zero_off, f"all-zero dout P={P} cin={cin} act={act}")


@pytest.mark.gpu
@pytest.mark.parametrize("P,cin", [(8391, 128), (8391, 64), (200, 128)])
def test_sparse_dout_exact_against_host(P, cin):
    """integer operands, act = 0 (every sum exact: tests/test_hip_head_proj.py), dout rows at 2 % density, switch on"""
    g = torch.Generator().manual_seed(P + cin)
    C = R.group_layout(3, cin, COUTS, "strided", BF16, False)["C"]
    y = R.ints((P, C), 4, g)
    ws = [R.ints((co, cin), 4, g) for co in COUTS]
    dout, _ = sparse_rows(P, 0.02, g, ints=True)
    pick = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)
    scale, invstd = pick[torch.randint(0, 3, (C,), generator=g)], pick[torch.randint(0, 3, (C,), generator=g)]
    shift, mean, mg, mgx = R.ints((C,), 2, g), R.ints((C,), 2, g), R.ints((C,), 3, g), R.ints((C,), 2, g)
    rig = Rig(P, cin, 0, y, dout, ws, scale, shift, mean, invstd, mg, mgx)
    rig.run(1)
    torch.cuda.synchronize()
    v = rig.views
    cov = torch.zeros(C, dtype=torch.bool)
    for o in rig.xoff:
        cov[o:o + cin] = True
    r = R.bn_bwd(y, dout, ws, rig.xoff, scale, shift, mean, invstd, 0)
    want = torch.zeros(rig.nrun, int(cov.sum()), 2, dtype=torch.float64)
    for b in range(rig.nrun):
        lo, hi = b * rig.ppb, min(P, (b + 1) * rig.ppb)
        if lo < hi:
            want[b, :, 0], want[b, :, 1] = r["g"][lo:hi][:, cov].sum(0), r["gx"][lo:hi][:, cov].sum(0)
    assert_exact(v["part"].double().cpu().view(rig.nrun, C, 2)[:, cov], want, f"mode 0 P={P} cin={cin}")
    assert bool(R.untouched(v["part"].view(rig.nrun, C, 2)[:, ~cov.to(DEV)]).all()), "mode 0 wrote an uncovered channel"
    assert_exact(v["dy"].double().cpu()[:, cov], R.rnd(R.bn_bwd_apply(r, scale, mg, mgx)[:, cov], torch.bfloat16), f"mode 1 P={P} cin={cin}")
    assert bool(R.untouched(v["dy"][:, ~cov.to(DEV)]).all()), "mode 1 wrote an uncovered channel"
    act = R.bn_act(y, scale, shift, 0, torch.bfloat16)
    dw, db, _, _ = R.proj_bwd_weight(act, dout, rig.xoff, COUTS, cin, comp=False)
    sl = v["slab"].double().cpu().view(rig.nblk, TOT, cin).sum(0)
    for br in range(3):
        assert_exact(v["dw"][br].double().cpu().view(COUTS[br], cin), dw[br], f"dW[{br}] P={P} cin={cin}")
        assert_exact(v["db"][br].double().cpu(), db[br], f"db[{br}] P={P} cin={cin}")
        assert_exact(sl[OOFF[br]:OOFF[br] + COUTS[br]], dw[br], f"slab rows of branch {br} P={P} cin={cin}")


@pytest.mark.gpu
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("P,cin", SHAPES)
def test_skipped_chunks_are_not_read(P, cin, act):
    g0 = torch.Generator().manual_seed(P + cin + 7)
    dout, _ = sparse_rows(P, 0.02, g0)
    dout[:, OOFF[2]] = 0                      # the one-output branch: no gradient at all
    rig, _ = real_rig(P, cin, act, dout)
    clean = rig.run(1)
    # NaN where the branch's 32-pixel chunk holds no dout value (chunks start at multiples of 32: every run starts at one of 64).
    # A run whose first 64 pixels are active in all four 16-pixel chunks is taken dense as a whole (projg_scan_run): no NaN there.
    n32 = -(-P // 32)
    pad = torch.zeros(n32 * 32, TOT)
    pad[:P] = dout
    ybad = rig.yd.clone()
    for br in range(3):
        cols = pad[:, OOFF[br]:OOFF[br] + COUTS[br]]
        idle = (cols.reshape(n32, -1) == 0).all(1)
        act16 = (cols.reshape(2 * n32, -1) != 0).any(1)
        rows = idle.repeat_interleave(32)[:P]
        for ppr in (rig.ppb, rig.wpb):
            for lo in range(0, P, ppr):
                if bool(act16[lo // 16:lo // 16 + 4].all()):
                    rows[lo:lo + ppr] = False
        assert bool(rows.any()) and (br == 2 or not bool(rows.all()))
        ybad[:, rig.xoff[br]:rig.xoff[br] + cin][rows.to(DEV)] = float("nan")
    keep = rig.yd.clone()
    rig.yd.copy_(ybad)
    on, off = rig.run(1), rig.run(0)
    rig.yd.copy_(keep)
    names = ["part", "slab", "bslab"] + [f"dw{br}" for br in range(3)] + [f"db{br}" for br in range(3)]
    for k in names:
        assert torch.equal(bits(on[k]), bits(clean[k])), f"`{k}`: a skipped chunk's y reached the result (P={P} cin={cin} act={act})"
        assert bool(torch.isfinite(written(on[k])).all()), k
    for k in ["part", "slab"] + [f"dw{br}" for br in range(3)]:
        assert bool(written(off[k]).isnan().any()), f"`{k}`: the dense path is expected to carry 0 * NaN (P={P} cin={cin} act={act})"
    # the apply pass still reads y there: NaN in, NaN out, in both positions
    assert bool(written(on["dy"]).isnan().any()) and bool(written(off["dy"]).isnan().any())
