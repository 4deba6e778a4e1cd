"""CPU: the references of proj_attn_ref.py pinned in float64 against torch.nn.functional (attention: softmax / matmul and autograd;
projections: F.conv2d and autograd; the folded BatchNorm: F.batch_norm and autograd), the case lists of tests/test_hip_attention.py
and tests/test_hip_head_proj.py checked for every boundary the kernels have, and the float32 distances that the attention bounds
are built on measured (DESIGN.md §4 quotes them)."""
import math

import pytest
import torch
import torch.nn.functional as F

import proj_attn_ref as R
from proj_attn_ref import BF16, F32


# ---------------------------------------------------------------------------------------------------------------- attention
def _rand_attn(B, N, nh, kd, hd, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, N, nh * (2 * kd + hd), generator=g, dtype=torch.float64),
            torch.randn(B, N, nh * hd, generator=g, dtype=torch.float64), torch.randn(B, N, nh * hd, generator=g, dtype=torch.float64))


@pytest.mark.parametrize("kd,hd", R.DIMS)
def test_attention_reference_is_softmax_matmul_and_its_autograd(kd, hd):
    B, N, nh, scale = 2, 37, 3, 0.23
    qkv, dout, extra = _rand_attn(B, N, nh, kd, hd, kd)
    x = qkv.clone().requires_grad_(True)
    t = R.heads(x, nh, 2 * kd + hd)
    q, k, v = t[..., :kd], t[..., kd:2 * kd], t[..., 2 * kd:]
    s = q @ k.transpose(-1, -2) * scale
    o = F.softmax(s, -1) @ v
    out = R.unheads(o)
    f = R.attn_fwd(qkv, nh, kd, hd, scale)
    assert torch.allclose(f["out"], out.detach(), rtol=1e-12, atol=1e-14)
    assert torch.allclose(f["lse"], torch.logsumexp(s, -1).detach(), rtol=1e-12, atol=1e-14)
    # loss = <out, dout> + <v, dv_extra>: the `pe` branch of PSA hands its gradient of v to the kernel as dv_extra
    ((out * dout).sum() + (R.unheads(v) * extra).sum()).backward()
    r = R.attn_bwd(qkv, f["out"], dout, extra, f["lse"], nh, kd, hd, scale)
    assert torch.allclose(r["dqkv"], x.grad, rtol=1e-10, atol=1e-13)
    assert torch.allclose(r["delta"], R.heads(dout * f["out"], nh, hd).sum(-1), rtol=1e-12, atol=1e-14)
    r0 = R.attn_bwd(qkv, f["out"], dout, None, f["lse"], nh, kd, hd, scale)
    d = R.blocks(r["dqkv"] - r0["dqkv"], nh, kd, hd)
    assert float(d["dq"].abs().max()) == 0 and float(d["dk"].abs().max()) == 0
    assert torch.allclose(R.unheads(d["dv"]), extra, rtol=0, atol=1e-14)
    # the companions dominate their results term by term
    assert bool((f["out_abs"] >= f["out"].abs() - 1e-14).all()) and bool((r["dqkv_abs"] >= r["dqkv"].abs() - 1e-12).all())
    assert bool((f["out_rnd"] <= 2.0 ** -8 * f["out_abs"] * 1.001).all()) and bool((f["out_rnd"] >= 2.0 ** -9 * f["out_abs"]).all())


@pytest.mark.parametrize("kd,hd", R.DIMS)
@pytest.mark.parametrize("N", [1, 17, 129])
@pytest.mark.parametrize("extra", [False, True])
def test_attention_exact_case_is_what_the_reference_computes(kd, hd, N, extra):
    """the closed-form expectations of attn_exact equal the float64 reference on the same inputs up to exp(-128); in fp32 the
    runner-up's weight exp(-128) IS zero, so there they are exact"""
    a = R.attn_exact(2, N, 2, kd, hd, extra)
    f = R.attn_fwd(a["qkv"], 2, kd, hd, 1.0)
    assert torch.allclose(f["out"], a["out"], rtol=0, atol=1e-40) and torch.allclose(f["lse"], a["lse"], rtol=0, atol=1e-40)
    r = R.attn_bwd(a["qkv"], a["out"], a["dout"], a["dv_extra"], a["lse"], 2, kd, hd, 1.0)
    assert torch.allclose(r["dqkv"], a["dqkv"], rtol=0, atol=1e-40) and torch.equal(r["delta"], a["delta"])
    assert float(torch.exp(torch.tensor(-128.0, dtype=torch.float32))) == 0.0
    t = R.heads(a["qkv"], 2, 2 * kd + hd)
    s = torch.einsum("bhid,bhjd->bhij", t[..., :kd], t[..., kd:2 * kd])
    top = s.topk(min(2, N), -1).values
    assert bool((top[..., 0] == 64.0 * kd).all()) and float(s.abs().max()) <= 64.0 * kd
    if N > 1:
        assert float((top[..., 0] - top[..., 1]).min()) >= 128
    assert bool((s.argmax(-1) == a["pi"]).all())
    for b in range(2):  # bijections, a different one per (image, head)
        for h in range(2):
            assert sorted(a["pi"][b, h].tolist()) == list(range(N))
    if N > 4:
        assert not torch.equal(a["pi"][0, 0], a["pi"][0, 1]) and not torch.equal(a["pi"][0, 0], a["pi"][1, 0])
    assert torch.equal(a["qkv"], a["qkv"].bfloat16().double()) and torch.equal(a["dqkv"], a["dqkv"].bfloat16().double())


def test_attention_exact_cases_reach_every_chunk_and_tile_edge():
    edges = {16: "MFMA 16-query / 16-key tile", 32: "MFMA 32-key step", 64: "VALU TK tile, 64-query MFMA block",
             128: "VALU 128-query block", 256: "bwd_kv chunk (36/72)", 512: "forward KC, bwd_kv chunk (32/64)", 1024: "bwd_q chunk"}
    assert R.AX_N == sorted(set(R.AX_N)) and 1 in R.AX_N and 1600 in R.AX_N
    for e, what in edges.items():
        assert {e - 1, e, e + 1} <= set(R.AX_N), what
    for route in R.AX_ROUTES:
        for kd, hd in R.DIMS:
            cs = [c for c in R.AX_CASES if c[0] == route and c[1:3] == (kd, hd)]
            assert [c[4] for c in cs] == R.AX_N
            assert {c[6] for c in cs} == {"dense", "strided"}
            assert all(c[3] * c[5] == 4 for c in cs if c[4] <= 129) and all(c[3] == 1 and c[5] in (1, 2) for c in cs if c[4] > 129)
            assert {c[5] for c in cs if c[4] > 129} == {1, 2}
            # both layouts on both sides of the largest chunk edges
            for lo, hi in ((511, 513), (1023, 1025)):
                assert {c[6] for c in cs if lo <= c[4] <= hi} == {"dense", "strided"}
    for N in R.AX_N:
        assert math.gcd(R.perm_mult(N), N) == 1
    assert set(R.AR_CASES) == {(kd, hd, k, N) for kd, hd in R.DIMS for k in ("randn", "peaked") for N in (77, 400, 513, 1025)}


def test_attention_float32_distances_and_tighter_than_before():
    """The fp32 allowance of the attention bounds is 4 x the distance printed here.  Condition: on every route the total bound on
    `out` is below a quarter of the old tests' 2e-2 max|ref| for at least 99 % of the elements of every case."""
    d = R.attn_f32_distance()
    print("float32 restatement distances (units of the companion sums):", {k: f"{v:.3e}" for k, v in d.items()})
    assert all(0 < v < 1e-4 for v in d.values()), d
    worst = {}
    for case in R.AR_CASES:
        a = R.attn_real(case)
        old = 2e-2 * float(a["ref"]["out"].abs().max())
        for route in ("f32", "valu", "mfma"):
            if route == "mfma":
                _, bound = R.attn_bound_mfma_out(case)
            else:
                bound = R.attn_bound(route, "out", a["ref"]["out"], a["comp"]["out"], a["crnd"]["out"], d)
            frac = float((bound < 0.25 * old).double().mean())
            worst[route] = min(worst.get(route, 1.0), frac)
            assert frac >= 0.99, f"{case} {route}: only {frac:.4f} of the `out` bounds are below a quarter of the old tolerance"
        # the MFMA forward's own statement stays inside the bound against plain float64 (its rounding of e is covered term by term)
        pr, _ = R.attn_bound_mfma_out(case)
        wide = R.attn_bound("mfma", "out", a["ref"]["out"], a["comp"]["out"], a["crnd"]["out"], d)
        assert bool(((pr - a["ref"]["out"]).abs() <= wide).all())
    print("smallest share of `out` bounds below a quarter of the old tolerance:", worst)


def test_flat_two_to_minus_nine_is_not_a_rounding_bound():
    """why the MFMA bounds sum half_ulp_bf16 per term: with p peaked, rounding e to bf16 alone moves `out` by more than
    2^-9 sum p |v| (1 + 2^-8 rounds to 1)"""
    assert float(torch.tensor(1 + 2.0 ** -8).bfloat16()) == 1.0
    over = 0
    for case in R.AR_CASES:
        a = R.attn_real(case)
        pr, _ = R.attn_bound_mfma_out(case)
        over += int(((pr - a["ref"]["out"]).abs() > 2.0 ** -9 * a["comp"]["out"]).sum())
    assert over > 0


def test_flip_zone():
    e = torch.tensor([1.0, 1 + 2.0 ** -8, 1 + 2.0 ** -8 + 1e-6, 1 + 2.0 ** -8 - 1e-6, 1.5, 2.0 ** -30], dtype=torch.float64)
    assert R.bf16_flip_zone(e, 1e-5).tolist() == [False, True, True, True, False, True]
    assert R.bf16_flip_zone(e, 1e-7).tolist() == [False, True, False, False, False, True]


# ---------------------------------------------------------------------------------------------------------------- projections
def _proj_inputs(P, nb, cin, couts, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(P, C, generator=g, dtype=torch.float64)
    ws = [torch.randn(c, cin, generator=g, dtype=torch.float64) for c in couts]
    bs = [torch.randn(c, generator=g, dtype=torch.float64) for c in couts]
    dy = torch.randn(P, sum(couts), generator=g, dtype=torch.float64)
    return x, ws, bs, dy


def test_projection_references_are_conv2d_and_its_autograd():
    P, cin, couts = 19, 12, (3, 1, 24, 9)
    xoff = [24, 0, 36, 48]  # not ascending, channels 12 .. 23 and 60 .. 63 uncovered
    C = 64
    x, ws, bs, dy = _proj_inputs(P, 4, cin, couts, C, 3)
    xg = x.clone().requires_grad_(True)
    wg = [w.clone().requires_grad_(True) for w in ws]
    bg = [b.clone().requires_grad_(True) for b in bs]
    ys = []
    for br in range(4):
        xin = xg[:, xoff[br]:xoff[br] + cin].t().reshape(1, cin, P, 1)
        ys.append(F.conv2d(xin, wg[br][:, :, None, None], bg[br]).reshape(couts[br], P).t())
    y = torch.cat(ys, 1)  # the running output offset is the concatenation
    (y * dy).sum().backward()
    yr, ya = R.proj_fwd(x, ws, bs, xoff)
    assert torch.allclose(yr, y.detach(), rtol=1e-12, atol=1e-13) and bool((ya >= yr.abs() - 1e-13).all())
    dx, _ = R.proj_bwd_data(dy, ws, xoff, C)
    cov = torch.zeros(C, dtype=torch.bool)
    for o in xoff:
        cov[o:o + cin] = True
    assert bool(dx[:, ~cov].isnan().all()) and torch.allclose(dx[:, cov], xg.grad[:, cov], rtol=1e-12, atol=1e-13)
    assert float(xg.grad[:, ~cov].abs().max()) == 0
    dw, db, dwa, _ = R.proj_bwd_weight(x, dy, xoff, couts, cin)
    for br in range(4):
        assert torch.allclose(dw[br], wg[br].grad, rtol=1e-12, atol=1e-13) and torch.allclose(db[br], bg[br].grad, rtol=1e-12, atol=1e-13)
        assert bool((dwa[br] >= dw[br].abs() - 1e-13).all())
    # two branches on one slice (forward only)
    y2, _ = R.proj_fwd(x, ws[:2], bs[:2], [24, 24])
    assert torch.allclose(y2[:, :3], x[:, 24:36] @ ws[0].t() + bs[0]) and torch.allclose(y2[:, 3:], x[:, 24:36] @ ws[1].t() + bs[1])


@pytest.mark.parametrize("act", [0, 1])
def test_batchnorm_projection_references_are_batch_norm_and_autograd(act):
    """proj(act(BN(y))) with the batch statistics: forward through F.batch_norm, backward through autograd; mode 0 is the pair of
    sums, mode 1 the gradient wrt y; the activation is rounded to the storage type (float64 here: no rounding)"""
    P, cin, couts, C, eps = 23, 8, (2, 24, 5), 32, 1e-3
    xoff = [16, 0, 24]
    y, ws, bs, dout = _proj_inputs(P, 3, cin, couts, C, 5 + act)
    g = torch.Generator().manual_seed(9)
    gamma, beta = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.randn(C, generator=g, dtype=torch.float64)
    yg = y.clone().requires_grad_(True)
    u = F.batch_norm(yg, None, None, gamma, beta, True, 0.1, eps)
    a = F.silu(u) if act else u
    out = torch.cat([a[:, xoff[br]:xoff[br] + cin] @ ws[br].t() + bs[br] for br in range(3)], 1)
    (out * dout).sum().backward()
    mean, invstd = y.mean(0), 1 / torch.sqrt(y.var(0, unbiased=False) + eps)
    scale = gamma * invstd
    shift = beta - mean * scale
    an = R.bn_act(y, scale, shift, act, torch.float64)
    assert torch.allclose(an, a.detach(), rtol=1e-12, atol=1e-13)
    yo, _ = R.proj_fwd(an, ws, bs, xoff)
    assert torch.allclose(yo, out.detach(), rtol=1e-12, atol=1e-13)
    r = R.bn_bwd(y, dout, ws, xoff, scale, shift, mean, invstd, act)
    cov = ~r["g"][0].isnan()
    assert int(cov.sum()) == 3 * cin
    mg, mgx = r["g"].sum(0) / P, r["gx"].sum(0) / P
    dy = R.bn_bwd_apply(r, scale, mg, mgx)
    assert torch.allclose(dy[:, cov], yg.grad[:, cov], rtol=1e-9, atol=1e-12)
    assert bool((r["g_abs"][:, cov] >= r["g"][:, cov].abs() - 1e-13).all())
    # the rounding to the storage type is a plain cast
    ab = R.bn_act(y.bfloat16().double(), scale.float().double(), shift.float().double(), act, torch.bfloat16)
    assert torch.equal(ab, ab.bfloat16().double()) and float((ab - an).abs().max()) < 0.1


def _wg_blocks(P):  # y3d_proj_group_blocks, y3d_proj_group_bwd_weight_bn_mfma_blocks
    return min(64, max(1, -(-P // 1024)))


def _runs128(P):  # y3d_proj_group_bn_bwd_blocks and the forward's run count
    return min(128, max(1, -(-P // 64)))


def test_projection_cases_reach_every_cap_edge_and_placement():
    want_p = {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 8191, 8192, 8193, 65537}
    assert set(R.PX_P) == want_p
    for cases, ip in ((R.PG_CASES, 1), (R.PM_CASES, 0)):
        assert {c[ip] for c in cases} >= want_p
        assert all(c[ip + 1] == 2 for c in cases if c[ip] == 65537) and all(c[ip + 1] in (1, 8, 16) for c in cases if c[ip] != 65537)
        assert {c[ip + 1] for c in cases} == {1, 2, 8, 16}
        assert any(c[ip + 2] == R.HEAD_COUTS * 2 for c in cases)
        assert all(len(c[ip + 2]) == c[ip + 1] for c in cases)
        assert {c[-1] for c in cases} == {"dense", "strided"}
        assert {c[-1] for c in cases if c[ip] == 65537} == {"dense", "strided"}
    pg_couts = {o for c in R.PG_CASES for o in c[3]}
    assert {1, 8, 9, 16, 17, 24} <= pg_couts and max(pg_couts) == 24
    for dt in (BF16, F32):  # the OG = 8 pass edges in both dtypes
        assert {1, 8, 9, 16, 17, 24} <= {o for c in R.PG_CASES if c[0] == dt for o in c[3]}
    assert {c[4] for c in R.PG_CASES if c[0] == BF16} == {8, 64, 80, 128, 256}
    assert {c[4] for c in R.PG_CASES if c[0] == F32} == {4, 68, 128}
    pm_couts = {o for c in R.PM_CASES for o in c[2]}
    assert {25, 32, 1, 16, 17, 24} <= pm_couts and {c[3] for c in R.PM_CASES} == {64, 128}
    # weight gradients: one block, several, the 64-block cap; cin % 64 != 0 with more than one block (the slab pitch is cin)
    assert {_wg_blocks(c[1]) for c in R.PG_CASES} >= {1, 2, 8, 9, 64}
    assert any(c[4] % 64 and _wg_blocks(c[1]) > 1 for c in R.PG_CASES if c[0] == BF16)
    assert any(c[4] % 64 and _wg_blocks(c[1]) > 1 for c in R.PG_CASES if c[0] == F32)
    # the four-pixels-in-flight loop (4 * PT pixels per trip: 128 bf16, 64 fp32) entered, left with single steps behind it, and skipped
    for dt, pt in ((BF16, 32), (F32, 16)):
        steps = set()
        for c in R.PG_CASES:
            if c[0] == dt:
                ppb = -(-c[1] // _wg_blocks(c[1]))
                steps.add((ppb > 3 * pt, (-(-ppb // pt)) % 4))
        assert (True, 0) in steps and any(e and r for e, r in steps) and any(not e for e, r in steps), (dt, steps)
    # bwd_data: 2048-block cap (256 threads, one 16-byte chunk each)
    assert any(c[1] * (c[4] // R.CE[c[0]]) > 2048 * 256 for c in R.PG_CASES)
    # MFMA weight gradient: 128-pixel rounding leaves empty trailing runs at 65537
    nrun = _wg_blocks(65537)
    ppb = -(-(-(-65537 // nrun)) // 128) * 128
    assert nrun == 64 and (nrun - 1) * ppb >= 65537
    # forward / bn_bwd runs: 128-run cap, empty trailing runs at 8193 (runs 65 .. 127 start past P)
    for P in (8193,):
        nr = _runs128(P)
        pp = -(-(-(-P // nr)) // 64) * 64
        assert nr == 128 and 65 * pp >= P > 64 * pp
    assert any(c[0] == 8193 for c in R.PR_CASES) and {c[0] for c in R.PR_CASES} == {65, 1025, 8193}
    assert {c[4] for c in R.PR_CASES} == {"bf16", "f32"} and {c[3] for c in R.PR_CASES} == {64, 128}
    # placement of the strided layout
    for dt in (BF16, F32):
        for fwd in (True, False):
            lay = R.group_layout(8, 64, R.take(R.EDGE_COUTS, 8), "strided", dt, fwd)
            xo = lay["xoff"]
            assert xo != sorted(xo) and all(o % R.CE[dt] == 0 for o in xo) and lay["xsw"] % R.CE[dt] == 0 and lay["dysw"] % 8 == 0
            assert (len(set(xo)) < len(xo)) == fwd                       # two branches on one slice: forward only
            assert lay["C"] > len(set(xo)) * 64 and max(xo) + 64 <= lay["C"]
            assert lay["xsw"] > lay["C"] and lay["ysw"] > 52 and lay["dsw"] > 52 and lay["dysw"] > lay["C"]
    # single-branch entries: the Cout <= 4 and the 24-wide kernels, both dtypes, one block and the 128-block cap, accumulate both ways
    assert {c[3] <= 4 for c in R.P1_CASES} == {True, False} and {c[0] for c in R.P1_CASES} == {BF16, F32}
    assert {min(128, -(-c[1] // 512)) for c in R.P1_CASES} >= {1, 2, 3, 16, 17, 128}
    assert {c[0] for c in R.SR_CASES} >= {1, 128} and any(c[1] % 256 for c in R.SR_CASES) and any(c[1] > 256 for c in R.SR_CASES)


def test_exact_projection_operands_stay_exact():
    """|x|, |dy|, |w|, |b| <= 4 (activations of the BatchNorm forms <= 4 * 2 + 2): every fp32 partial sum is an integer multiple of
    1/2 below 2^24, whatever the order"""
    assert 65537 * 4 * 10 * 2 < 2 ** 24 and 256 * 10 * 4 * 2 + 8 < 2 ** 24
    g = torch.Generator().manual_seed(0)
    x = R.ints((1000,), 4, g)
    assert float(x.abs().max()) == 4 and torch.equal(x, x.bfloat16().double())
