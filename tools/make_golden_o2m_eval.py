"""Mints tests/golden/head3d_o2m_eval_k33.npz and head3d_o2m_eval_k31.npz from the REFERENCE: the eval-mode one-to-many forward of
`v10Detect3d` (`_forward`, head.py:800-812) and the validator's `postprocess` with `use_o2m_depth` (models/yolov10_3D/val.py:33-59),
run on the CPU.

    python tools/make_golden_o2m_eval.py      # needs the reference checkout (oracle.ref_shim.import_reference) and scikit-learn

As shipped the reference's eval `forward` returns no "one2many" entry, so the switch raises KeyError there; the validator unpacks
`preds["one2many"][0]`, which is what `_forward` returns in eval mode, and the tool hands `postprocess` exactly that.

Recipe (oracle/make_golden.py's head fixtures: nc = 3, ch = (16, 32, 64), every branch 16 wide, layouts (k1, k2, nl) = (3, 3, 3) and
(3, 1, 2), B = 2, maps 32^2 / 16^2 / 8^2), changed so that the fusion stage has work to do: after `bias_init` the `s2d` projection bias
is 40 (boxes wide enough for neighbouring anchors to overlap above 0.9), the `dep` projection weights are multiplied by 30 (votes
spread over metres), and `o2m_heads` = a deep copy of `o2o_heads` plus 0.05 * randn on every parameter.

Stored per layout: `x`, the one-to-one `y`, `_forward`'s `y_m` and `maps_m` (from an eval deep copy of its own: the one-to-one call
leaves padding = 0 behind), the reference's `rowsO` (2, 50, 37) and `rowsM` (2, 250, 37), `fused` = `postprocess`'s output, the
versions of scikit-learn, numpy and torch as integers, and the seed; next to it head3d_o2m_eval_<tag>_state.npz with the state of
`o2o_heads.*` / `o2m_heads.*`.  To keep every file under 1 MiB: parameters, BatchNorm buffers and `x` are rounded to
bf16-representable float32 values BEFORE the reference runs (the low mantissa bits then compress; the reference computes in float32
on exactly the stored numbers), and since the decode leaves all but channels nc .. nc + 6 of a map untouched, `maps_m` is stored as
those six raw channels over all anchors (`maps_m_raw` (B, 6, A)): level map = `y_m`'s anchors of the level with them put back
(tests/o2m_eval_ref.py `load`).

The tool asserts, on the reference's numbers only, what the tests rely on (tests/val_tail_ref.py's `fusion_rows`):
  * at most 5 % of the fused rows have a margin <= TAU_MIXED;
  * at least half of the rows have >= 3 voters, and over the two files at least one row has <= 1;
  * no IoU lies within 1e-6 of 0.9, no vote weight exp(-u) within 1e-3 of 0.1;
  * `oracle.restate.kde_fuse_depth(rowsO, rowsM)` equals the validator's output bit for bit;
  * no two rows of an image have the same score and the last anchor kept is not tied with the first one dropped (the reference's
    top-k leaves the order of ties open; the kernels take the lowest index).
A seed that misses a condition is skipped for the next one; the conditions are never loosened.  The fixtures hold data only."""
from __future__ import annotations

import copy
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_shim as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
LAYOUTS = (("k33", 3, 3, 3), ("k31", 3, 1, 2))
CH, NC, B, MAX_DET = (16, 32, 64), 3, 2, 50
SIZES = (32, 16, 8)
FIRST_SEED, TRIES = 5, 40


def set_bn(m, gen):
    """initialize_weights' eps / momentum and randomised affine / running statistics, as oracle/make_golden.py sets them"""
    import torch
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.eps, mod.momentum = 1e-3, 0.03
            with torch.no_grad():
                mod.weight.copy_(1.0 + 0.2 * (torch.rand(mod.weight.shape, generator=gen) - 0.5))
                mod.bias.copy_(0.2 * (torch.rand(mod.bias.shape, generator=gen) - 0.5))
                mod.running_mean.copy_(0.1 * (torch.rand(mod.bias.shape, generator=gen) - 0.5))
                mod.running_var.copy_(1.0 + 0.5 * torch.rand(mod.bias.shape, generator=gen))


def version_ints(v):
    return np.array([int("".join(c for c in p if c.isdigit()) or 0) for p in v.split("+")[0].split(".")[:3]], np.int64)


def mint(k1, k2, nl, seed):
    """-> the arrays of one layout at one seed"""
    import torch
    from ultralytics.models.yolov10_3D.val import YOLOv10_3DDetectionValidator as Validator
    from ultralytics.nn.modules.head import v10Detect3d
    from ultralytics.utils import ops as ref_ops
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    chan = {k + "_c": 16 for k in ("cls", "o2d", "s2d", "o3d", "s3d", "hd", "dep", "dep_un")}
    hd = v10Detect3d(NC, CH, False, chan, False, False, False, False, nl, False, False, k1, k2)
    hd.stride = torch.tensor([8.0, 16.0, 32.0][:nl])
    hd.bias_init()
    with torch.no_grad():
        for i in range(nl):
            hd.s2d[i][-1].bias.fill_(40.0)
            hd.dep[i][-1].weight.mul_(30.0)
    set_bn(hd, g)
    hd.o2m_heads = copy.deepcopy(hd.o2o_heads)
    with torch.no_grad():
        for p in hd.o2m_heads.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g))
    with torch.no_grad():  # bf16-representable values (see above)
        for t in list(hd.parameters()) + [b for b in hd.buffers() if b.is_floating_point()]:
            t.copy_(t.bfloat16().float())
    state = {f"model.0.{k}": v.clone() for k, v in hd.state_dict().items() if k.startswith(("o2o_heads.", "o2m_heads."))}
    xe = [torch.randn(B, CH[i], SIZES[i], SIZES[i], generator=g).bfloat16().float() for i in range(nl)]
    with torch.no_grad():
        y, _ = copy.deepcopy(hd).eval()([x.clone() for x in xe])["one2one"]
        (y_m, maps_m), _, _ = copy.deepcopy(hd).eval()._forward([x.clone() for x in xe])
    A = sum(s * s for s in SIZES[:nl])
    assert tuple(y.shape) == (B, NC + 35, A) == tuple(y_m.shape) and len(maps_m) == nl
    flat_m = torch.cat([m.reshape(B, NC + 35, -1) for m in maps_m], 2)
    other = [c for c in range(NC + 35) if not NC <= c < NC + 6]
    assert torch.equal(flat_m[:, other], y_m[:, other]), "the decode changed a channel outside nc .. nc + 6"

    def rows(t, k):
        reg, scores, labels = ref_ops.v10_3Dpostprocess(t.transpose(-1, -2), k, NC)
        return torch.cat((reg, scores.unsqueeze(-1), labels.unsqueeze(-1)), dim=-1)

    rowsO, rowsM = rows(y, MAX_DET), rows(y_m, MAX_DET * 5)
    ns = types.SimpleNamespace(args=types.SimpleNamespace(use_o2m_depth=True, use_dino_depth=False, max_det=MAX_DET), nc=NC)
    ns.aggregate_o2m_preds = lambda o, m, thres=0.1: Validator.aggregate_o2m_preds(ns, o, m, thres)
    with torch.no_grad():
        fused = Validator.postprocess(ns, {"one2one": (y.clone(), None), "one2many": (y_m.clone(), [m.clone() for m in maps_m])})
    assert tuple(rowsO.shape) == (B, MAX_DET, 37) and tuple(rowsM.shape) == (B, MAX_DET * 5, 37) and fused.shape == rowsO.shape
    return {"x": xe, "state": state, "y": y, "y_m": y_m, "maps_m_raw": flat_m[:, NC:NC + 6].contiguous(), "rowsO": rowsO.float(), "rowsM": rowsM.float(),
            "fused": fused.float(), "meta": np.array([k1, k2, nl]), "seed": np.array(seed)}


def conditions(d):
    """the tool's conditions on one layout's arrays -> (list of the ones missed, statistics)"""
    import torch
    import val_tail_ref as V
    from oracle import restate as RS
    O, M, fused = d["rowsO"], d["rowsM"], d["fused"]
    rows = V.fusion_rows(O, M, V.THRES, V.IOU_THRES, 500)
    n = np.array([r["n"] for r in rows])
    nf, under, smallest = V.fusion_stats(rows, V.TAU_MIXED)
    iou = torch.stack([V.box_iou_xyxy(O[b, :, :4], M[b, :, :4]) for b in range(O.shape[0])])
    d_iou = float((iou.double() - 0.9).abs().min())
    w = torch.exp(-torch.cat((O[..., -3].flatten(), M[..., -3].flatten())).double())
    d_w = float((w - 0.1).abs().min())
    restated = RS.kde_fuse_depth(O, M, V.THRES, V.IOU_THRES, 500)
    missed = []
    ties = sum(int(t[b, :, 35].unique().numel() != t.shape[1]) for t in (O, M) for b in range(t.shape[0]))
    for t, yy in ((O, d["y"]), (M, d["y_m"])):
        best = yy[:, :NC].amax(1).sort(1, descending=True)[0]
        ties += int((best[:, t.shape[1] - 1] == best[:, t.shape[1]]).sum())
    if ties:
        missed.append(f"{ties} ties among the scores")
    if nf == 0 or under > 0.05 * nf:
        missed.append(f"{under} of {nf} fused rows have a margin <= {V.TAU_MIXED:g}")
    if (n >= 3).sum() * 2 < n.size:
        missed.append(f"only {(n >= 3).sum()} of {n.size} rows have >= 3 voters")
    if d_iou <= 1e-6:
        missed.append(f"an IoU lies {d_iou:.2e} from 0.9")
    if d_w <= 1e-3:
        missed.append(f"a vote weight lies {d_w:.2e} from 0.1")
    if not torch.equal(restated.view(torch.int32), fused.contiguous().view(torch.int32)):
        missed.append("oracle.restate.kde_fuse_depth differs from the validator's output")
    stats = {"fused": nf, "rows": int(n.size), "voters": (int(n.min()), int(np.median(n)), int(n.max())), "under_tau": under,
             "smallest_margin": smallest, "iou_gap": d_iou, "weight_gap": d_w, "lonely": int((n <= 1).sum())}
    return missed, stats


def main():
    import sklearn
    import torch
    R.import_reference()
    for seed in range(FIRST_SEED, FIRST_SEED + TRIES):
        made, ok = {}, True
        for tag, k1, k2, nl in LAYOUTS:
            d = mint(k1, k2, nl, seed)
            missed, stats = conditions(d)
            print(f"seed {seed} {tag}: {stats}" + (f"  MISSED: {missed}" if missed else ""))
            made[tag] = (d, stats)
            ok = ok and not missed
        if ok and not any(s["lonely"] for _, s in made.values()):
            print(f"seed {seed}: no row with <= 1 voter in either file")
            ok = False
        if ok:
            break
    else:
        raise SystemExit(f"no seed in {FIRST_SEED}..{FIRST_SEED + TRIES - 1} meets the conditions")
    os.makedirs(OUT, exist_ok=True)
    for tag, (d, _) in made.items():
        state = d.pop("state")
        spath = os.path.join(OUT, f"head3d_o2m_eval_{tag}_state.npz")
        np.savez_compressed(spath, **{f"state/{k}": v.detach().numpy() for k, v in state.items()})
        assert os.path.getsize(spath) < 1024 * 1024, os.path.getsize(spath)
        print(f"wrote {spath} ({os.path.getsize(spath)} bytes)")
        flat = {"sklearn_version": version_ints(sklearn.__version__), "numpy_version": version_ints(np.__version__),
                "torch_version": version_ints(torch.__version__)}
        for k, v in d.items():
            if isinstance(v, dict):
                flat.update({f"{k}/{kk}": vv.detach().numpy() for kk, vv in v.items()})
            elif isinstance(v, (list, tuple)):
                flat.update({f"{k}/{j}": vv.detach().numpy() for j, vv in enumerate(v)})
            else:
                flat[k] = v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)
        path = os.path.join(OUT, f"head3d_o2m_eval_{tag}.npz")
        np.savez_compressed(path, **flat)
        size = os.path.getsize(path)
        assert size < 1024 * 1024, size
        print(f"wrote {path} ({size} bytes)")


if __name__ == "__main__":
    main()
