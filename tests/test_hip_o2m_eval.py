"""GPU: the one-to-many depth vote at eval (`use_o2m_depth`) stage by stage against the reference's fixtures
(tests/o2m_eval_ref.py): the head's dense one-to-many forward on both of its routes, the row chain behind `raw_rows3d` on the
reference's own head outputs, its refusals, the `y3d_rows_depth_from_map` kernel against a NumPy restatement kept here, and the
switches of `Validator3d` / `Predictor3d` on seeded models against the hand-chained public calls."""
import os

import numpy as np
import pytest
import torch

import o2m_eval_ref as F
import tail_ref as R
import val_tail_ref as V
from kitti_labels_tree import fixture as tree_fixture, write_tree

import yolov10_3d_amd as y3d
from yolov10_3d_amd import graph, kitti, kitti_eval, predict, val
from yolov10_3d_amd import modules as M
from yolov10_3d_amd import ops as P_ops
from yolov10_3d_amd._lib import Y3DError

pytestmark = pytest.mark.gpu
DEV = "cuda"
RES = (320, 256)
FRAMES = [0, 2, 6, 7, 9]


@pytest.fixture(autouse=True)
def _float32_compute():
    before = P_ops.compute_dtype()
    y3d.set_compute_dtype(torch.float32)
    yield
    y3d.set_compute_dtype(before)


def rel_err(a, b, floor=1e-4):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    return ((a - b).abs().max() / b.abs().max().clamp(min=floor)).item()


def bits_equal(a, b):
    bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else R.bits(t)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a.detach().cpu().contiguous()), bits(b.detach().cpu().contiguous()))


# ---------------------------------------------------------------------------------------------------------------- 1. the head
def fixture_head(g):
    k1, k2, nl = [int(v) for v in g["meta"]]
    chan = {k + "_c": 16 for k in ("cls", "o2d", "s2d", "o3d", "s3d", "hd", "dep", "dep_un")}
    hd = M.v10Detect3d(3, (16, 32, 64), False, chan, False, False, False, False, nl, False, False, k1, k2)
    hd.stride = torch.tensor([8.0, 16.0, 32.0][:nl])
    sd = {k[len("model.0."):]: v for k, v in g["state"].items()}
    missing, unexpected = hd.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.split(".")[0] in ("cls", "o2d", "s2d", "o3d", "s3d", "hd", "dep", "dep_un") for k in missing), (missing, unexpected)
    for m in hd.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eps, m.momentum = 1e-3, 0.03
    return hd.to(DEV).eval(), (k1, k2, nl)


@pytest.mark.parametrize("tag", F.TAGS)
def test_head_one2many_against_the_reference(tag):
    """exact-fp32 mode: `maps_m` and `y_m` of the dense one-to-many forward within 1e-3 relative of the reference's `_forward`, every
    level once on the stacked route and once on the module route; the one-to-one entry bit-equal with the switch on and off; the
    switch-off dict has today's keys; the modules' paddings are as before"""
    g = F.load(tag)
    hd, (k1, k2, nl) = fixture_head(g)
    xs = [x.to(DEV) for x in g["x"]]
    pads = lambda: [tuple(m.conv.padding) for m in hd.modules() if isinstance(m, M.Conv)]
    pads0 = pads()
    stacked = []
    inner = hd._dense_stacked
    hd._dense_stacked = lambda plan, heads, i, xi: (stacked.append(i), inner(plan, heads, i, xi))[1]
    try:
        for generic, want_stacked in ((False, list(range(nl))), (True, [])):
            hd.generic = generic
            del stacked[:]
            with torch.no_grad():
                hd.eval_one2many = False
                off = hd(xs)
                hd.eval_one2many = True
                on = hd(xs)
            route = "module" if generic else "stacked"
            assert stacked == want_stacked, f"{route} route: levels {stacked} ran on the stacks"
            assert list(off) == ["one2one", "o2o_embs"] and off["o2o_embs"] is None
            assert list(on) == ["one2one", "o2o_embs", "one2many"]
            assert bits_equal(on["one2one"][0], off["one2one"][0]) and all(bits_equal(a, b) for a, b in zip(on["one2one"][1], off["one2one"][1]))
            y_m, maps_m = on["one2many"]
            assert y_m.dtype == torch.float32 and len(maps_m) == nl
            errs = [rel_err(a, b) for a, b in zip(maps_m, g["maps_m"])] + [rel_err(y_m, g["y_m"])]
            print(f"\n[o2m head] {tag} {route}: relative errors of the level maps and y_m {['%.2e' % e for e in errs]}")
            assert max(errs) <= 1e-3, f"{tag} {route} route: {errs}"
            assert pads() == pads0
    finally:
        del hd._dense_stacked
        hd.generic = False
    assert pads0.count((k1 // 2, k1 // 2)) >= 16 * nl and hd.o2m_heads[1][0][0].conv.padding == (k1 // 2, k1 // 2)
    # the one-to-many branches gone: an error, not a silent one-to-one answer
    gone = hd.o2m_heads
    del hd.o2m_heads
    try:
        with pytest.raises(Y3DError, match="no one-to-many branches"):
            hd(xs)
    finally:
        hd.o2m_heads = gone


# ---------------------------------------------------------------------------------------------------------------- 2. the row chain
@pytest.mark.parametrize("tag", F.TAGS)
def test_row_chain_on_the_references_outputs(tag):
    """the function behind `raw_rows3d` on the reference's y and y_m (no conv rounding): rowsO / rowsM are the reference's (labels and
    selection exactly - the score column is a gather, so bit-equal - values within 1e-6) at K = 50 and KM = 250; the fused rows pass
    `val_tail_ref.check_fusion` at TAU_MIXED and are the reference's pick wherever its margin exceeds tau"""
    g = F.load(tag)
    fused, rowsO, rowsM = predict.o2m_rows3d(g["y"].to(DEV), g["y_m"].to(DEV), F.MAX_DET, F.NC)
    torch.cuda.synchronize()
    for got, ref, k, what in ((rowsO, g["rowsO"], F.MAX_DET, "rowsO"), (rowsM, g["rowsM"], F.KM, "rowsM")):
        got = got.cpu()
        assert tuple(got.shape) == (2, k, 37) == tuple(ref.shape) and got.dtype == torch.float32
        assert torch.equal(got[..., 36], ref[..., 36]), f"{what}: labels differ"
        assert bits_equal(got[..., 35], ref[..., 35]), f"{what}: another selection (scores differ)"
        err = float(((got - ref).abs() / ref.abs().clamp(min=1.0)).max())
        print(f"\n[o2m rows] {tag} {what}: largest deviation {err:.3e}")
        assert err <= 1e-6, f"{what}: {err:.3e}"
    rows = F.fusion_rows(tag)
    fused = fused.cpu()
    worst, off_pick = V.check_fusion(fused, g["rowsO"], rows, V.TAU_MIXED, tag)
    clear = torch.tensor([r["n"] > 1 and r["margin"] > V.TAU_MIXED for r in rows]).reshape(2, F.MAX_DET)
    nf = sum(r["n"] > 1 for r in rows)
    assert int(clear.sum()) >= 0.95 * nf
    assert bits_equal(fused[..., 33][clear], g["fused"][..., 33][clear]), "a fused depth is not the reference's where its margin exceeds tau"
    lonely = torch.tensor([r["n"] <= 1 for r in rows]).reshape(2, F.MAX_DET)
    assert bits_equal(fused[..., 33][lonely], g["rowsO"][..., 33][lonely])
    print(f"[o2m rows] {tag}: {nf} fused rows, {int(clear.sum())} with a clear margin, {off_pick} off the reference's pick, largest "
          f"log-density gap {worst:.3e}")


# ---------------------------------------------------------------------------------------------------------------- 3. refusals
class HeadModel(torch.nn.Module):
    """a head alone behind the model interface `raw_rows3d` reads"""

    def __init__(self, head):
        super().__init__()
        self.model, self.yaml, self.calls = torch.nn.ModuleList([head]), {"nc": head.nc}, 0

    def forward(self, img):
        self.calls += 1
        B, _, H, W = img.shape
        head = self.model[-1]
        chs = [head.o2o_heads[0][i][0].conv.in_channels for i in range(head.nl)]
        return head([torch.ones(B, c, H // s, W // s, device=img.device) for c, s in zip(chs, (8, 16, 32))])


def n3d_head(**kw):
    """the 3D head of yolov10n_3D.yaml: inputs of 64 / 128 / 256 channels"""
    cfg = y3d.yaml_model_load("yolov10n_3D.yaml")
    head = y3d.YOLOv10_3DDetectionModel(cfg).model[-1]
    if kw:
        args = dict(nc=head.nc, ch=[head.cls[i][0].conv.in_channels for i in range(3)], channels={k + "_c": getattr(head, k)[0][0].conv.out_channels for k in head.output_channels})
        head = M.v10Detect3d(**args, **kw)
        head.stride = torch.tensor([8.0, 16.0, 32.0])
    return HeadModel(head.to(DEV).eval())


def test_refusals_before_any_launch():
    """max_det * 5 above the anchors (N-3D head on maps 8^2 / 4^2 / 2^2 = 84 anchors: max_det 50 and 17 ask for 250 and 85 rows) and
    above the fusion kernel's 3902 rows (max_det 781) are refused before the forward; 16 (80 rows) passes the row chain; a head with
    `use_predecessors` keeps raising"""
    m = n3d_head()
    img = torch.zeros(2, 3, 64, 64, device=DEV)
    for max_det, match in ((50, "84 anchors"), (17, "84 anchors"), (781, "at most 3902")):
        with pytest.raises(Y3DError, match=match):
            predict.raw_rows3d(m, img, max_det, use_o2m_depth=True)
    assert m.calls == 0 and m.model[-1].eval_one2many is False
    gen = torch.Generator().manual_seed(0)
    yO, yM = (torch.randn(2, 38, 84, generator=gen).to(DEV) for _ in range(2))
    for max_det in (50, 17):
        with pytest.raises(Y3DError, match="84 anchors"):
            predict.o2m_rows3d(yO, yM, max_det, 3)
    with pytest.raises(Y3DError, match="at most 3902"):
        predict.o2m_rows3d(torch.zeros(1, 38, 4000, device=DEV), torch.zeros(1, 38, 4000, device=DEV), 781, 3)
    fused, rowsO, rowsM = predict.o2m_rows3d(yO, yM, 16, 3)
    assert tuple(fused.shape) == (2, 16, 37) and tuple(rowsM.shape) == (2, 80, 37) and bool(torch.isfinite(fused).all())
    # use_predecessors: no eval path, with the switch as without it
    p = n3d_head(use_predecessors=True)
    big = torch.zeros(1, 3, 256, 320, device=DEV)
    for flag in (False, True):
        with pytest.raises(RuntimeError, match="use_predecessors has no eval path"):
            with torch.no_grad():
                predict.raw_rows3d(p, big, 50, use_o2m_depth=flag)
    assert p.model[-1].eval_one2many is False


# ---------------------------------------------------------------------------------------------------------------- 4. the kernel
def depth_from_map_ref(rows, dmap):
    """`y3d_rows_depth_from_map` on NumPy float32 arrays: rows (B, K, C), dmap (B, Hm, Wm) -> rows with column C - 4 read from the map"""
    out, (B, K, C), (Hm, Wm) = rows.copy(), rows.shape, dmap.shape[1:]
    with np.errstate(invalid="ignore"):
        idx = lambda c, dim: np.trunc(np.where(c >= 0, np.minimum(c, np.float32(dim - 1)), np.float32(0))).astype(np.int64)
        out[..., C - 4] = dmap[np.arange(B)[:, None], idx(rows[..., 5], Hm), idx(rows[..., 4], Wm)]
    return out


def map_case(B, K, C, Hm, Wm, seed):
    """rows with random columns and centres all over and outside the map; the first centres of every image are the edge values:
    negative, -0.5, exact integers, n + 0.999, dim - 1, dim, 1e20, NaN (and the infinities), paired with each other"""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((B, K, C)).astype(np.float32) * 50
    rows[..., 4] = rng.uniform(-3, Wm + 3, (B, K)).astype(np.float32)
    rows[..., 5] = rng.uniform(-3, Hm + 3, (B, K)).astype(np.float32)
    edge = lambda dim: np.array([-7.0, -0.5, -0.0, 0.0, 1.0, dim // 2, dim // 2 + 0.999, dim - 1, dim - 1 + 0.999, dim, dim + 0.5, 1e20, np.nan,
                                 np.inf, -np.inf, -1e20], np.float32)
    ex, ey = edge(Wm), edge(Hm)
    n = min(K, ex.size)
    rows[:, :n, 4] = ex[:n]
    rows[:, :n, 5] = np.roll(ey, 5)[:n]
    if K > 2 * ex.size:
        rows[:, n:2 * n, 4] = np.roll(ex, 3)[:n]
        rows[:, n:2 * n, 5] = ey[:n]
    dmap = rng.uniform(1, 80, (B, Hm, Wm)).astype(np.float32)
    return rows, dmap


MAP_CASES = [(1, 1, 37, 1, 1), (2, 257, 37, 7, 9), (3, 50, 8, 96, 320), (2, 257, 37, 1, 1), (1, 1, 37, 96, 320), (3, 50, 8, 7, 9)]


@pytest.mark.parametrize("B,K,C,Hm,Wm", MAP_CASES)
def test_rows_depth_from_map_bit_equal(B, K, C, Hm, Wm):
    rows, dmap = map_case(B, K, C, Hm, Wm, seed=B * 1000 + K + Hm)
    want = torch.from_numpy(depth_from_map_ref(rows, dmap))
    rd, md = torch.from_numpy(rows).to(DEV), torch.from_numpy(dmap).to(DEV)
    n = B * K * C
    buf = R.sentinel(n + 256, torch.float32, DEV)
    out = buf[:n].view(B, K, C)
    y3d.lib().rows_depth_from_map(rd.data_ptr(), B, K, C, md.data_ptr(), Hm, Wm, out.data_ptr(), P_ops.stream())
    torch.cuda.synchronize()
    assert bool(R.untouched(buf[n:]).all()), "a store went past the end of the output"
    assert bits_equal(out, want), "the C ABI and the restatement disagree"
    assert bits_equal(kitti.depth_from_map(rd, md), want) and bits_equal(rd, torch.from_numpy(rows)), "the wrapper disagrees or changed its input"
    # a strided view is handled (through a dense copy), as the wrapper documents
    wide = torch.full((B, K, C + 3), 9.0, device=DEV)
    wide[..., :C] = rd
    tall = torch.zeros(B, Hm, Wm + 2, device=DEV)
    tall[..., :Wm] = md
    assert bits_equal(kitti.depth_from_map(wide[..., :C], tall[..., :Wm]), want)


def test_rows_depth_from_map_refuses_without_writing():
    L, st = y3d.lib(), P_ops.stream()
    rows, dmap = torch.zeros(2, 5, 37, device=DEV), torch.ones(2, 4, 6, device=DEV)
    n = 2 * 5 * 37
    buf = R.sentinel(n + 512, torch.float32, DEV)
    out = buf[:n]
    r, m, o = rows.data_ptr(), dmap.data_ptr(), out.data_ptr()
    bad = [((None, 2, 5, 37, m, 4, 6, o), "null"), ((r, 2, 5, 37, None, 4, 6, o), "null"), ((r, 2, 5, 37, m, 4, 6, None), "null"),
           ((r, 2, 5, 7, m, 4, 6, o), "C >= 8"), ((r, 0, 5, 37, m, 4, 6, o), "bad sizes"), ((r, 2, 0, 37, m, 4, 6, o), "bad sizes"),
           ((r, 2, 5, 37, m, 0, 6, o), "bad sizes"), ((r, 2, 5, 37, m, 4, 0, o), "bad sizes"),
           ((o, 2, 5, 37, m, 4, 6, o), "overlaps"), ((o + 4 * 36, 1, 1, 37, m, 4, 6, o), "overlaps"), ((r, 2, 5, 37, o + 16, 4, 6, o), "overlaps"),
           ((r, 2, 5, 37, o + 4 * n - 4 * 47, 4, 6, o), "overlaps")]
    for args, match in bad:
        with pytest.raises(Y3DError, match=match):
            L.rows_depth_from_map(*args, st)
    torch.cuda.synchronize()
    assert bool(R.untouched(buf).all()), "a refused call wrote to its output"
    with pytest.raises(Y3DError, match="rows_depth_from_map"):  # no rows
        kitti.depth_from_map(torch.zeros(2, 0, 37, device=DEV), dmap)
    # inputs that end exactly where the output begins do not overlap it
    whole = torch.zeros(3 * n, device=DEV)
    L.rows_depth_from_map(whole.data_ptr(), 2, 5, 37, m, 4, 6, whole.data_ptr() + 4 * n, st)
    torch.cuda.synchronize()
    assert bool((whole[n:2 * n].view(2, 5, 37)[..., 33] == 1).all()) and float(whole[2 * n:].abs().sum()) == 0.0


def test_rows_depth_from_map_replays_from_a_graph():
    """one capture at the default queue settings; replayed on new rows and a new map it gives the bits of the eager call"""
    B, K, C, Hm, Wm = 2, 257, 37, 7, 9
    rows0, map0 = map_case(B, K, C, Hm, Wm, seed=1)
    rows1, map1 = map_case(B, K, C, Hm, Wm, seed=2)
    g = graph.GraphedForward(kitti.depth_from_map, torch.from_numpy(rows0).to(DEV), torch.from_numpy(map0).to(DEV))
    assert bits_equal(g(torch.from_numpy(rows0).to(DEV), torch.from_numpy(map0).to(DEV)), torch.from_numpy(depth_from_map_ref(rows0, map0)))
    assert bits_equal(g(torch.from_numpy(rows1).to(DEV), torch.from_numpy(map1).to(DEV)), torch.from_numpy(depth_from_map_ref(rows1, map1)))
    assert g.captures == 1


# ---------------------------------------------------------------------------------------------------------------- 5. model level
def _prime(m, shape):
    """tests/test_hip_validators.py's: BatchNorm statistics of a random batch and wider random score projections"""
    bns = [b for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)]
    keep = [b.momentum for b in bns]
    for b in bns:
        b.momentum = 1.0
    head = m.model[-1]
    with torch.no_grad():
        m.train()(torch.rand(*shape, device=DEV))
        for branch in (head.cls, head.dep_un):
            for level in branch:
                level[-1].weight.normal_(0.0, 0.05)
                level[-1].bias.add_(torch.randn_like(level[-1].bias))
    for b, mom in zip(bns, keep):
        b.momentum = mom
    P_ops.bump_param_epoch()
    return m


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    r = write_tree(str(tmp_path_factory.mktemp("kitti_o2m")), tree_fixture(), images=True)
    open(os.path.join(r, "ImageSets", "val.txt"), "w").write("".join(f"{i:06d}\n" for i in FRAMES))
    return r


@pytest.fixture(scope="module")
def model3d():
    """seeded yolov10n_3D at 320 x 256 (1 680 anchors, 80 cells on the stride-32 level).  After the constructor the one-to-many set is
    the one-to-one set, so the fused depth would be the row's own: the one-to-many set restarts as a copy of the primed one-to-one
    set with seeded noise on its depth branch - boxes, classes and depth variances stay equal, so every row has voters"""
    before = P_ops.compute_dtype()
    y3d.set_compute_dtype(torch.float32)
    torch.manual_seed(3)
    m = y3d.YOLOv10_3DDetectionModel(y3d.yaml_model_load("yolov10n_3D.yaml")).to(DEV)
    _prime(m, (2, 3, RES[1], RES[0]))
    head = m.model[-1]
    gen = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for a, b in zip(head.o2m_heads.state_dict().values(), head.o2o_heads.state_dict().values()):
            a.copy_(b)
        for p in head.o2m_heads[6].parameters():
            p.add_((0.05 * torch.randn(p.shape, generator=gen)).to(DEV))
    P_ops.bump_param_epoch()
    y3d.set_compute_dtype(before)
    return m.eval()


def hand_rows(model, img, max_det=50):
    """the public calls of the one-to-many chain, by hand: img (B, H, W, 3) uint8 -> fused rows"""
    head = model.model[-1]
    head.eval_one2many = True
    try:
        with torch.no_grad():
            out = model(img.permute(0, 3, 1, 2))
    finally:
        head.eval_one2many = False
    rowsO, rowsM = predict.rows3d(out["one2one"][0], max_det, 3), predict.rows3d(out["one2many"][0], max_det * 5, 3)
    return kitti.aggregate_o2m_preds(rowsO, rowsM)


def hand_results(root, model, rows_of, conf):
    results = {}
    for s in range(0, len(FRAMES), 2):
        idx = list(range(s, min(s + 2, len(FRAMES))))
        b = kitti.build_batch(root, idx, kitti.data_args(), DEV, mode="val", compact=True, resolution=RES)
        raw = rows_of(b["img"])
        calib = torch.tensor([kitti.calib_params(kitti.read_calib(os.path.join(root, "training/calib", f"{FRAMES[p]:06d}.txt"))) for p in idx],
                             dtype=torch.float64)
        results.update(kitti.decode_preds(raw, calib, b["im_file"], b["ratio_pad"], [i["trans_inv"] for i in b["info"]], threshold=conf))
    return results


CONF = 0.001


def test_validator3d_one2many_equals_the_hand_chain(root, model3d):
    want = hand_results(root, model3d, lambda img: hand_rows(model3d, img), CONF)
    plain = val.Validator3d(model3d, root, batch=2, conf=CONF, resolution=RES)
    plain()
    assert list(plain._graphs) == []
    for use_graph in (False, True):
        v = val.Validator3d(model3d, root, batch=2, conf=CONF, resolution=RES, graph=use_graph, use_o2m_depth=True)
        res = v()
        assert model3d.model[-1].eval_one2many is False and not model3d.training
        assert v.results == want, f"graph={use_graph}: the validator's rows are not the hand chain's"
        assert float(res["metrics/3D"]) == float(kitti_eval.get_stats(want, os.path.join(root, "training", "label_2")))
        if use_graph:
            assert sorted(v._graphs) == [((1, RES[1], RES[0], 3), "o2m"), ((2, RES[1], RES[0], 3), "o2m")]
            assert all(g.captures == 1 for g in v._graphs.values())
    # against the switch-off run: the same rows kept, class, 2D box, h w l and score bit-equal, some depth moved
    assert list(v.results) == list(plain.results)
    moved = total = 0
    for f in v.results:
        a, b = np.array(v.results[f], np.float64).reshape(-1, 14), np.array(plain.results[f], np.float64).reshape(-1, 14)
        assert a.shape == b.shape
        same = [0, 2, 3, 4, 5, 6, 7, 8, 13]
        assert a[:, same].tobytes() == b[:, same].tobytes(), f
        moved, total = moved + int((a[:, 11] != b[:, 11]).sum()), total + len(a)
    print(f"\n[o2m model] {moved} of {total} kept rows changed their z")
    assert total > 0 and moved >= 1


def test_predictor3d_one2many_equals_the_hand_chain(root, model3d):
    rng = np.random.default_rng(5)
    images = [rng.integers(0, 256, (375, 1242, 3), dtype=np.uint8), rng.integers(0, 256, (370, 1224, 3), dtype=np.uint8)]
    P2s = [kitti.read_calib(os.path.join(root, "training/calib", f"{i:06d}.txt")) for i in (0, 2)]
    on = predict.Predictor3d(model3d, conf=CONF, resolution=RES, use_o2m_depth=True)
    off = predict.Predictor3d(model3d, conf=CONF, resolution=RES)
    got, plain = on(images, P2s, static=True), off(images, P2s, static=True)
    assert model3d.model[-1].eval_one2many is False
    p = on.plan([im.shape[:2] for im in images], P2s)
    img = kitti.augment_images([torch.from_numpy(im).to(DEV) for im in images], [None] * 2, [False] * 2, list(p["trans_inv"]), RES, "uint8")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    want = predict.predict3d_rows(hand_rows(model3d, img), up(p["calib6"]), up(p["P2"]), up(p["ratio"]), up(p["trans_inv"]), CONF)
    assert all(bits_equal(a, b) for a, b in zip(got, want))
    assert bits_equal(got[3], plain[3]) and int(got[3].sum()) > 0 and not bits_equal(got[0], plain[0])


def test_dino_depth_reads_the_ramp_and_one2many_wins(root, model3d):
    H, W = RES[1], RES[0]
    calls = []

    def ramp(img):
        calls.append((tuple(img.shape), img.dtype, torch.is_grad_enabled()))
        B = img.shape[0]
        base = torch.arange(H * W, dtype=torch.float32, device=img.device).reshape(1, H, W) + 1.0
        return base + 100000.0 * torch.arange(B, dtype=torch.float32, device=img.device).reshape(B, 1, 1), None

    b = kitti.build_batch(root, [0, 1], kitti.data_args(), DEV, mode="val", compact=True, resolution=RES)
    img = b["img"].permute(0, 3, 1, 2)
    with torch.no_grad():
        base = predict.raw_rows3d(model3d, img, 50)
        rows = predict.raw_rows3d(model3d, img, 50, depth_maps=ramp(img)[0])
        both = predict.raw_rows3d(model3d, img, 50, use_o2m_depth=True, depth_maps=ramp(img)[0])
    keep = [c for c in range(37) if c != 33]
    assert bits_equal(rows[..., keep], base[..., keep])
    cx, cy = base[..., 4].cpu().numpy(), base[..., 5].cpu().numpy()
    ix, iy = np.clip(np.trunc(cx), 0, W - 1), np.clip(np.trunc(cy), 0, H - 1)
    want = (iy * W + ix + 1.0 + 100000.0 * np.arange(2)[:, None]).astype(np.float32)
    assert np.array_equal(rows[..., 33].cpu().numpy(), want)
    assert bits_equal(both, hand_rows(model3d, b["img"]))  # one-to-many wins: the maps are not read
    # the validator: the callable runs per batch on the image, outside the graph, under no_grad; rows as the hand chain's
    del calls[:]
    want_res = hand_results(root, model3d, lambda im: predict.raw_rows3d(model3d, im.permute(0, 3, 1, 2), 50, depth_maps=ramp(im.permute(0, 3, 1, 2))[0]), CONF)
    del calls[:]
    for use_graph in (False, True):
        v = val.Validator3d(model3d, root, batch=2, conf=CONF, resolution=RES, graph=use_graph, use_dino_depth=True, depth_fn=ramp)
        v()
        assert v.results == want_res
        assert calls == [((2, 3, H, W), torch.uint8, False)] * 2 + [((1, 3, H, W), torch.uint8, False)]
        del calls[:]
    no_call = lambda img: (_ for _ in ()).throw(AssertionError("the depth callable ran although one-to-many wins"))
    w = val.Validator3d(model3d, root, batch=2, conf=CONF, resolution=RES, use_o2m_depth=True, use_dino_depth=True, depth_fn=no_call)
    w()
    assert w.results == hand_results(root, model3d, lambda im: hand_rows(model3d, im), CONF)


# ---------------------------------------------------------------------------------------------------------------- 6. M-3D
def test_m3d_one2many_routes_agree():
    """yolov10m_3D (cls wider than the regression branches: not the uniform layout) at 256 x 256: the eval forward with the switch
    within 1e-3 of the same forward on the module route"""
    torch.manual_seed(6)
    m = y3d.YOLOv10_3DDetectionModel(y3d.yaml_model_load("yolov10m_3D.yaml")).to(DEV).eval()
    head = m.model[-1]
    with torch.no_grad():
        for p in head.o2m_heads.parameters():
            p.add_(0.02 * torch.randn_like(p))
    P_ops.bump_param_epoch()
    img = torch.rand(1, 3, 256, 256, device=DEV)
    head.eval_one2many = True
    outs = {}
    for generic in (False, True):
        head.generic = generic
        with torch.no_grad():
            outs[generic] = m(img)
    head.generic, head.eval_one2many = False, False
    (y, maps), (y_ref, maps_ref) = outs[False]["one2many"], outs[True]["one2many"]
    assert not any(head._stacks(i).uniform for i in range(head.nl))  # the "wide cls" layout: its dense forward is the module route's
    assert tuple(y.shape) == (1, head.no, sum((256 // int(s)) ** 2 for s in head.stride.tolist())) and bool(torch.isfinite(y).all())
    errs = [rel_err(a, b) for a, b in zip(maps, maps_ref)] + [rel_err(y, y_ref)]
    print(f"\n[o2m M-3D] relative errors against the module route {['%.2e' % e for e in errs]}")
    assert max(errs) <= 1e-3
    assert not bits_equal(outs[False]["one2many"][0], outs[False]["one2one"][0])
