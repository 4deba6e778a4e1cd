"""GPU: the two kernels of hierarchical task learning - `y3d_htl_update` (csrc/htl.hip) and `y3d_loss3d_weighted` (csrc/tal_loss3d.hip).

y3d_htl_update replays every loss sequence of tests/htl_ref.py on state placed inside a sentinel-filled buffer with guard words around every
part, and is compared with the FLOAT64 restatement.  The bound is 4 x max(d_ref, 6 x 2^-23): d_ref is the distance between the reference's
own float32 outputs (tests/golden/htl.npz) and the float64 restatement, computed at run time from the fixture (never from the device);
6 x 2^-23 is the spacing of float32 at the largest weight, 6, times 1.5; the factor 4 allows for host and device powf each being a few ulp
off.  Calls whose weights are ratios of small integers (all before epoch 6; 0 ** 0 = 1) must equal the fixture bit for bit.

y3d_loss3d_weighted runs on two `loss_ref` cases made here (the table of tests/loss_ref.py has no shape this small): B = 2, nc = 1, one
8 x 8 level; B = 4, nc = 3, the three levels of a 64 x 64 image (336 anchors: two blocks, the second partly filled).  Everything is compared
bit for bit with `y3d_loss3d` on the same inputs: a multiply by a weight is one fp32 operation, rounded once, and the host does the same."""
import ctypes

import numpy as np
import pytest
import torch

import htl_ref as H
import loss_ref as LR
import tail_ref as TR

pytestmark = pytest.mark.gpu

import yolov10_3d_amd as y3d  # noqa: E402
from yolov10_3d_amd import loss as PL, ops, train  # noqa: E402
from yolov10_3d_amd._lib import Y3DError  # noqa: E402

DEV = "cuda"
GUARD = 8


# ---- 1. y3d_htl_update ----------------------------------------------------------------------------------------------------------------------
class State:
    """ring (S x 12), init_diff, weights and the three int words, each between GUARD sentinel words of one fp32 buffer.  The ring, init_diff
    and the weights START as sentinels (NaN with a payload): a read of a row the ring does not hold yet would show in the weights."""

    def __init__(self, S):
        self.S = S
        sizes = {"ring": S * 12, "init_diff": 12, "weights": 12, "count": 1, "have_init": 1, "status": 1}
        pos, self.at = GUARD, {}
        for k, n in sizes.items():
            self.at[k] = (pos, n)
            pos += n + GUARD
        self.buf = TR.sentinel((pos,), torch.float32, DEV)
        gap = torch.ones(pos, dtype=torch.bool)
        for o, n in self.at.values():
            gap[o:o + n] = False
        self.gap = gap.to(DEV)
        for k in ("count", "have_init", "status"):
            self.part(k).view(torch.int32).zero_()

    def part(self, k):
        o, n = self.at[k]
        return self.buf[o:o + n]

    def ptr(self, k):
        return self.part(k).data_ptr()

    def update(self, items, tv, S=None, null=()):
        p = {k: (None if k in null else self.ptr(k)) for k in self.at}
        y3d.lib().htl_update(None if "items" in null else items.data_ptr(), float(tv), self.S if S is None else S, p["ring"], p["count"],
                             p["init_diff"], p["have_init"], p["weights"], p["status"], ops.stream())

    def ints(self):
        return {k: int(self.part(k).view(torch.int32).cpu()) for k in ("count", "have_init", "status")}

    def guards_intact(self):
        return bool(TR.untouched(self.buf[self.gap]).all())


def replay(epochs, losses, S=5):
    st = State(S)
    rows, status = [], []
    dev_losses = torch.from_numpy(np.ascontiguousarray(losses)).to(DEV)
    for i, e in enumerate(epochs):
        st.update(dev_losses[i], H.time_value(int(e)))
        rows.append(st.part("weights").cpu().numpy().copy())
        status.append(st.ints()["status"])
    return np.stack(rows), status, st


@pytest.fixture(scope="module")
def bound():
    b = 4 * max(H.d_ref(H.load_golden()), 6 * 2.0 ** -23)
    print(f"device bound {b:.3e}")
    return b


def check_rows(got, w64, bound, what):
    assert np.array_equal(np.isnan(got), np.isnan(w64)) and np.array_equal(np.isinf(got), np.isinf(w64)), f"{what}: non-finite pattern\n{got}\n{w64}"
    fin = np.isfinite(w64)
    d = float(np.abs(got.astype(np.float64) - w64)[fin].max())
    print(f"{what}: largest distance to the float64 restatement {d:.3e} (bound {bound:.3e})")
    assert d <= bound, f"{what}: {d:.3e} > {bound:.3e}"
    return d


@pytest.mark.parametrize("name", list(H.SEQUENCES))
def test_update_replays_the_sequences(name, bound):
    epochs, losses = H.SEQUENCES[name]
    got, status, st = replay(epochs, losses)
    w64, _ = H.run(epochs, losses, np.float64)
    check_rows(got, w64, bound, name)
    gw = H.load_golden()[name]["weights"]
    for r in H.exact_rows(name):
        assert np.array_equal(got[r].view(np.int32), gw[r].view(np.int32)), f"{name} call {r}: {got[r]} vs the reference's {gw[r]}"
    # the status bit: set by the first call with a non-finite weight, and it stays
    bad = [not np.isfinite(r).all() for r in w64]
    assert status == [int(any(bad[:i + 1])) for i in range(len(bad))], (status, bad)
    assert {"restart_inf": 1, "constant": 1}.get(name, 0) == status[-1]
    ints = st.ints()
    assert ints["count"] == 5 and ints["have_init"] == 1
    # the ring holds the last five losses, oldest first
    assert np.array_equal(st.part("ring").cpu().numpy().reshape(5, 12), losses[len(epochs) - 5:])
    assert st.guards_intact(), "a store went outside the state"


@pytest.mark.parametrize("S", [3, 8])
def test_update_with_other_ring_lengths(S, bound):
    """the shortest and the longest ring the launcher takes (one difference; six), against the restatement with that stat_epoch_nums"""
    k = np.arange(14)[:, None]
    rate = np.array([0.30, 0.10, 0.05, 0.12, 0.22, 0.08, 0.26, 0.11, 0.04, 0.13, 0.2, 0.07])
    losses = (H.BASE * (0.35 + 0.65 * np.exp(-rate * k * (1 + 0.05 * k)))).astype(np.float32)
    epochs = list(range(3, 17))
    got, status, st = replay(epochs, losses, S)
    wt = H.Weightor(np.float64, stat_epochs=S)
    w64 = np.stack([wt.compute_weight(l, e) for e, l in zip(epochs, losses)])
    assert (w64[S][2:6] > 0).all() or epochs[S] <= 5
    check_rows(got, w64, bound, f"stat_epochs {S}")
    assert not any(status) and st.ints() == {"count": S, "have_init": 1, "status": 0}
    assert np.array_equal(st.part("ring").cpu().numpy().reshape(S, 12), losses[-S:]) and st.guards_intact()


def test_update_refusals_leave_the_state_alone():
    st = State(5)
    items = torch.ones(12, device=DEV)
    before = st.buf.clone()
    for bad in ("items", "ring", "count", "init_diff", "have_init", "weights", "status"):
        with pytest.raises(Y3DError, match="htl_update"):
            st.update(items, 0.5, null=(bad,))
    for S in (2, 9, 0, -1):
        with pytest.raises(Y3DError, match="stat_epochs"):
            st.update(items, 0.5, S=S)
    torch.cuda.synchronize()
    assert torch.equal(TR.bits(st.buf), TR.bits(before))


def test_htl_weights_object_and_its_state_dict():
    """train.HtlWeights makes the same launches on its own buffer; a state_dict taken mid-way continues in a new object bit for bit; the table
    keeps its address"""
    epochs, losses = H.SEQUENCES["decay"]
    want, _, _ = replay(epochs, losses)
    dl = torch.from_numpy(losses).to(DEV)
    hw = train.HtlWeights(DEV)
    addr = hw.table.data_ptr()
    got = []
    for i, e in enumerate(epochs[:7]):
        assert hw.update(dl[i], e).data_ptr() == addr
        got.append(hw.table.cpu().numpy().copy())
    sd = hw.state_dict()
    assert sd["count"] == 5 and sd["have_init"] == 1 and sd["status"] == 0 and all(not v.is_cuda for v in sd.values() if torch.is_tensor(v))
    hw2 = train.HtlWeights(DEV)
    hw2.load_state_dict(sd)
    for i, e in list(enumerate(epochs))[7:]:
        hw2.update(dl[i], e)
        got.append(hw2.table.cpu().numpy().copy())
    assert np.array_equal(np.stack(got).view(np.int32), want.view(np.int32))
    assert int(hw2.status.cpu()) == 0
    with pytest.raises(Y3DError, match="12 loss items"):
        hw.update(dl[0].cpu(), 0)
    with pytest.raises(NotImplementedError, match="htl"):
        train.HtlWeights("cpu")


# ---- 2. y3d_loss3d_weighted -----------------------------------------------------------------------------------------------------------------
LR.BOXES.setdefault("htl_b2", [[(24, 28, 30, 26), (44, 40, 24, 28)], [(32, 32, 40, 36)]])
LR.BOXES.setdefault("htl_b4", [[(24, 28, 30, 26), (44, 40, 24, 28)], [(32, 32, 40, 36), (14, 50, 20, 18)], [(40, 22, 34, 30)],
                               [(20, 20, 28, 28), (46, 44, 26, 30), (30, 48, 22, 20)]])
CASES = {"b2_nc1_nl1": LR._case("htl_b2_nc1_nl1", "3d", (64, 64), (8.0,), 1, 8, "htl_b2", "B = 2, nc = 1, one level: 128 anchors, half a block"),
         "b4_nc3_nl3": LR._case("htl_b4_nc3_nl3", "3d", (64, 64), LR.S3, 3, 8, "htl_b4", "B = 4, nc = 3, 64 + 16 + 4 anchors per image: 336, two blocks")}
ITEM_GROUPS = {0: ("o2d", "s2d"), 1: ("cls",), 2: ("dep", "unc"), 3: ("o3d",), 4: ("s3d",), 5: ("hbin", "hres")}  # item -> groups of LR.groups3d
GENERAL = [0.37, 1.9, 0.0061, 2.5e-3, 1.3, 0.81]


def item_of_channel(nc):
    out = []
    for name, width in LR.groups3d(nc):
        out += [next(j for j, g in ITEM_GROUPS.items() if name in g)] * width
    return torch.tensor(out)


class Run:
    """one case on the device: padded targets, maps and a sentinel-filled gradient buffer per level with guards (made per call)"""

    def __init__(self, cname, dname, upcast=False):
        self.case = CASES[cname]
        self.dtype = torch.float32 if upcast else LR.DTYPES[dname]
        batch, self.B = LR.make_batch(self.case)
        maps = LR.make_maps(self.case, LR.DTYPES[dname])  # fp32 host tensors holding values of the storage type
        y3d.set_compute_dtype(self.dtype)
        self.crit = PL.DDDetectionLoss(LR.model_of(self.case), tal_topk=self.case["topk"])
        self.db = {k: v.to(DEV) for k, v in batch.items()}
        self.maps = [ops._dense_any(m.to(DEV), self.dtype) for m in maps]
        H_, W_ = maps[0].shape[2:]
        self.gt, self.n_used = self.crit.targets(self.db, self.B, H_, W_, DEV)
        PL.check_target_overflow(wait=True)
        self.no = self.case["nc"] + 35

    def __call__(self, table=None, store=True):
        """-> (items (6,), rows per level (B, H, W, no) fp32-or-bf16 host tensors or None, total or None, fg)"""
        maps, no, B = self.maps, self.no, self.B
        Hs, Ws = [m.shape[2] for m in maps], [m.shape[3] for m in maps]
        bufs = [TR.sentinel((B * h * w * no + 2 * GUARD,), self.dtype, DEV) for h, w in zip(Hs, Ws)]
        esz = bufs[0].element_size()
        cfg = self.crit.cfg(len(maps))
        assert cfg.item_w is None and cfg.store_grads
        if table is not None:
            cfg = cfg._replace(item_w=table, store_grads=store)
        r = PL._loss3d_set(cfg, self.gt.float().contiguous(), self.n_used, self.db["calib"].float().contiguous(), self.db["mean_sizes"].float().contiguous(),
                           PL.Levels([m.data_ptr() for m in maps], [m.stride(3) for m in maps], Hs, Ws, cfg.strides),
                           [b.data_ptr() + GUARD * esz for b in bufs] if store else None, [no] * len(maps), B, self.dtype, DEV)
        torch.cuda.synchronize()
        for b in bufs:
            assert bool(TR.untouched(b[:GUARD]).all() and TR.untouched(b[-GUARD:]).all()), "a gradient row went outside its map"
        rows = [b[GUARD:-GUARD].view(B, h, w, no).cpu() for b, h, w in zip(bufs, Hs, Ws)]
        if store:
            assert not any(bool(TR.untouched(x).any()) for x in rows), "an anchor's row was not written"
        return r.items.cpu(), rows, (r.total.cpu() if r.total is not None else None), r.fg.cpu()


def fold(items, w):
    a = 0.0
    for j in range(6):
        a += float(np.float64(np.float32(w[j]))) * float(items[j])
    return np.float32(a)


def table_of(w):
    return torch.tensor(w, dtype=torch.float32, device=DEV)


def same_bits(a, b):
    return torch.equal(TR.bits(a), TR.bits(b))


@pytest.fixture(scope="module", params=[(c, d) for c in CASES for d in ("fp32", "bf16")], ids=lambda p: f"{p[0]}-{p[1]}")
def plain(request):
    """y3d_loss3d itself on a case (made once, never changed)"""
    cname, dname = request.param
    run = Run(cname, dname)
    items, rows, total, fg = run()
    assert total is None and fg.any() and torch.isfinite(items).all() and (items > 0).all()
    if cname == "b4_nc3_nl3":
        assert fg.numel() == 336
    return cname, dname, run, items, rows


def test_weighted_with_ones_is_the_plain_entry(plain):
    cname, dname, run, items, rows = plain
    it, rw, total, _ = run(table_of([1.0] * 6))
    assert same_bits(it, items)
    assert all(same_bits(a, b) for a, b in zip(rw, rows))
    assert total.shape == (1,) and np.float32(total[0]) == fold(items, [1.0] * 6)


def test_weighted_rows_are_the_plain_rows_times_the_item_weight(plain):
    cname, dname, run, items, rows = plain
    it, rw, total, _ = run(table_of(GENERAL))
    assert same_bits(it, items), "the items must stay unweighted"
    assert np.float32(total[0]) == fold(items, GENERAL)
    w = torch.tensor(GENERAL, dtype=torch.float32)[item_of_channel(run.case["nc"])]
    if dname == "fp32":
        for lvl, (a, b) in enumerate(zip(rw, rows)):
            c0 = 0
            for name, width in LR.groups3d(run.case["nc"]):
                sl = slice(c0, c0 + width)
                c0 += width
                assert same_bits(a[..., sl], b[..., sl] * w[sl]), f"level {lvl} group {name}"
                assert bool(b[..., sl].any()), f"level {lvl} group {name}: the plain rows are all zero, the case shows nothing"
    else:
        # bf16 rows are rounded once, after the weight: the fp32 entry on the up-cast maps gives the unrounded rows
        up = Run(cname, dname, upcast=True)
        it32, rows32, _, _ = up()
        for lvl, (a, b) in enumerate(zip(rw, rows32)):
            assert same_bits(a, (b * w).to(torch.bfloat16)), f"level {lvl}"
        y3d.set_compute_dtype(run.dtype)


def test_a_zero_weight_zeroes_exactly_its_group(plain):
    cname, dname, run, items, rows = plain
    nc = run.case["nc"]
    item = item_of_channel(nc)
    for j in range(6):
        w = [1.0] * 6
        w[j] = 0.0
        it, rw, total, _ = run(table_of(w))
        assert same_bits(it, items) and np.float32(total[0]) == fold(items, w)
        for a, b in zip(rw, rows):
            assert not a[..., item == j].any(), f"item {j}: its channels must be exactly 0"
            assert same_bits(a[..., item != j], b[..., item != j]), f"item {j}: another item's channels changed"


def test_no_rows_without_a_gradient_buffer(plain):
    cname, dname, run, items, rows = plain
    it, rw, total, _ = run(table_of(GENERAL), store=False)
    assert all(bool(TR.untouched(x).all()) for x in rw)
    assert same_bits(it, items) and np.float32(total[0]) == fold(items, GENERAL)


def test_weighted_refusals(plain):
    cname, dname, run, items, rows = plain
    L = y3d.lib()
    maps = run.maps
    nl = len(maps)
    PV = ctypes.c_void_p * nl
    c_maps = PV(*[m.data_ptr() for m in maps])
    c_psw, c_gsw = (ctypes.c_int64 * nl)(*[m.stride(3) for m in maps]), (ctypes.c_int64 * nl)(*[run.no] * nl)
    c_H, c_W = (ctypes.c_int * nl)(*[m.shape[2] for m in maps]), (ctypes.c_int * nl)(*[m.shape[3] for m in maps])
    c_st = (ctypes.c_float * nl)(*run.case["strides"])
    t = table_of(GENERAL)
    out = torch.zeros(8, device=DEV)
    bufs = [TR.sentinel((run.B * m.shape[2] * m.shape[3] * run.no,), run.dtype, DEV) for m in maps]

    def call(grads, item_w, total):
        L.loss3d_weighted(ops.code(run.dtype), nl, c_maps, c_psw, grads, c_gsw, c_H, c_W, c_st, run.B, run.case["nc"], None, 1, None, None, None, None,
                          1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, None, None, item_w, total, ops.stream())

    with pytest.raises(Y3DError, match="item_w"):
        call(PV(*[b.data_ptr() for b in bufs]), None, out.data_ptr())
    with pytest.raises(Y3DError, match="item_w"):
        call(PV(*[b.data_ptr() for b in bufs]), t.data_ptr(), None)
    holes = [b.data_ptr() for b in bufs]
    holes[-1] = None
    with pytest.raises(Y3DError, match="grads"):
        call(PV(*holes), t.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert all(bool(TR.untouched(b).all()) for b in bufs) and not out.any()


# ---- 3. the criterion's route ----------------------------------------------------------------------------------------------------------------
def test_criterion_takes_the_table_and_none_restores_the_calls():
    """DDDetectionLoss with a table: loss = total (not times B), items unweighted, gradient = rows times the weight; under no_grad no row
    buffer; None: the calls of before"""
    run = Run("b4_nc3_nl3", "fp32")
    crit, B = run.crit, run.B

    def go(no_grad=False):
        dm = [m.clone().requires_grad_(True) for m in run.maps]
        with (torch.no_grad() if no_grad else torch.enable_grad()):
            loss, items = crit(dm, run.db)
            if not no_grad:
                loss.backward()
        return loss.detach().cpu(), items.cpu(), [m.grad.cpu() if m.grad is not None else None for m in dm]

    l0, i0, g0 = go()
    assert abs(float(l0) - B * float(i0.sum())) < 1e-5 * float(l0)
    t = table_of(GENERAL)
    crit.set_item_weights(t)
    assert crit.cfg(3).item_w is t
    l1, i1, g1 = go()
    assert same_bits(i1, i0) and np.float32(l1) == fold(i0, GENERAL)
    w = torch.tensor(GENERAL)[item_of_channel(3)].view(1, -1, 1, 1)
    for a, b in zip(g1, g0):
        assert same_bits(a, (b / B) * w)  # g0 = rows * B exactly (B = 4 is a power of two)
    t.copy_(torch.tensor([1.0] * 6))  # the table is read at every call: new contents, same tensor
    l2, i2, g2 = go()
    assert np.float32(l2) == fold(i0, [1.0] * 6) and all(torch.equal(a, b / B) for a, b in zip(g2, g0))
    l3, i3, g3 = go(no_grad=True)
    assert same_bits(i3, i0) and l3 == l2 and all(g is None for g in g3) and not l3.requires_grad
    crit.set_item_weights(None)
    assert crit.cfg(3).item_w is None
    l4, i4, g4 = go()
    assert l4 == l0 and same_bits(i4, i0) and all(same_bits(a, b) for a, b in zip(g4, g0))
    with pytest.raises(Y3DError, match="set_item_weights"):
        crit.set_item_weights(torch.ones(6))
    with pytest.raises(Y3DError, match="set_item_weights"):
        crit.set_item_weights(torch.ones(5, device=DEV))
