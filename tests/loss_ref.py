"""TEST INFRASTRUCTURE - float64 reference of the loss terms, margin checks of the assignment and the shared case table for
tests/test_hip_losses.py (device) and tests/test_loss_ref_host.py (host).  Plain torch; imports the oracle only, never the HIP library.

Two references, kept apart because they fail differently:

* the ASSIGNMENT (fg_mask, target_gt_idx, target_scores) is the oracle's: `oracle.restate.tal3d` / `tal2d` in fp32 (`assign3d` / `assign2d`
  below prepare their inputs exactly as `restate.loss3d_one` / `loss2d_one` do).  A top-k over fp32 metrics is only determined where the
  metrics are further apart than host and device libm disagree, so `assignment_margin` measures, on the oracle's own tensors, how far
  every decision of a case is from flipping; every case of the table must clear `MARGIN_FLOOR` (asserted on the host for each case).
* the LOSS ITEMS and their GRADIENT: `loss3d_terms` / `loss2d_terms`, the formulae of `restate.loss3d_one` / `loss2d_one`
  (utils/loss.py:82-113, 206-257, 821-963, 1112-1136) in float64, with the assignment as an INPUT; the gradient is torch.autograd's.

Measured on the host over all cases of the table (tests/test_loss_ref_host.py prints and bounds both):
  METRIC_ROUNDING = 2.2e-5: the largest relative difference between the oracle's fp32 alignment metric (and its tie-breaking "overlaps") and
      the same quantity in float64, over the entries that take part in a decision (the k + 1 largest of a box's row, the two largest of a
      multiply-selected anchor's column);
  MARGIN_FLOOR = 16 x METRIC_ROUNDING = 3.5e-4 (the device's libm differs from the host's by a few ulp per call, the metric chains ~10 calls).
"""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from oracle import restate as RS

METRIC_ROUNDING = 2.2e-5
MARGIN_FLOOR = 3.5e-4

GAINS3D = ("loss2d", "cls", "depth", "offset3d", "size3d", "heading")
GAINS2D = ("box", "cls", "dfl")
MODES = {"default": dict(tal_2d=True, tal_3d=True, kps_dist_metric="l1", constrain_anchors=True),
         "box_only": dict(tal_2d=True, tal_3d=False, kps_dist_metric="l1", constrain_anchors=True),
         "kps_only_l2": dict(tal_2d=False, tal_3d=True, kps_dist_metric="l2", constrain_anchors=True)}
KITTI_MEAN = [[1.76255119, 0.66068622, 0.84422524], [1.52563191, 1.62856739, 3.88311640], [1.73698127, 0.59706367, 1.76282397]]


def groups3d(nc):
    return [("cls", nc), ("o2d", 2), ("s2d", 2), ("o3d", 2), ("s3d", 3), ("hbin", 12), ("hres", 12), ("dep", 1), ("unc", 1)]


def groups2d(nc):
    return [("l", 16), ("t", 16), ("r", 16), ("b", 16), ("cls", nc)]


# ---------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------
def _grid64():
    """64 small boxes on an 8 x 8 grid of a 320 x 320 image (sizes vary a little so that no two boxes are congruent)"""
    return [(20.5 + 40 * i, 19.5 + 40 * j, 27 + (i * 3 + j) % 5, 26 + (i + j * 3) % 7) for j in range(8) for i in range(8)]


TINY = (98.0, 98.0, 2.0, 2.0)  # anchor centres sit at 4+8k, 8+16k, 16+32k: none lies inside (97, 99)^2
BOXES = {
    # per image: [(cx, cy, w, h) in pixels]; labels run 0, 1, 2, ... % nc over the rows, so they cover every class
    "normal": [[(96, 104, 88, 72), (212, 204, 120, 96), (150, 84, 56, 100)], [(170, 150, 150, 130), (70, 236, 96, 84)]],
    "normal256": [[(80, 90, 72, 60), (170, 160, 100, 84), (120, 60, 48, 80)], [(130, 120, 120, 110), (60, 190, 80, 70)]],
    "kitti": [[(640, 200, 520, 70), (300, 190, 44, 300), (1000, 220, 180, 120)], [(200, 100, 300, 50), (900, 200, 60, 280), (1150, 300, 150, 90)]],
    "hires": [[(400, 420, 300, 260), (900, 800, 420, 380), (640, 300, 160, 240), (250, 1000, 280, 200), (1000, 250, 200, 180)]],
    "empty_image": [[(96, 104, 88, 72), (212, 204, 120, 96)], [], [(170, 150, 150, 130), (70, 236, 96, 84), (230, 90, 70, 90)]],
    "tiny": [[TINY, (212, 204, 120, 96), (150, 84, 56, 100)], [(170, 150, 150, 130), (70, 236, 96, 84)]],
    "no_fg": [[TINY, (130.0, 98.0, 2.0, 2.0)], [(98.0, 162.0, 2.0, 2.0)]],
    "dup_nested": [[(120, 120, 100, 90), (120, 120, 100, 90), (134, 126, 100, 90)], [(160, 160, 200, 180), (160, 160, 120, 110), (160, 160, 60, 50)]],
    "border": [[(20, 160, 80, 100), (250, 300, 100, 90), (160, 150, 90, 80)], [(300, 20, 90, 70), (150, 170, 120, 100)]],
    "capacity": [_grid64(), [(170, 150, 150, 130)]],
    "big": [[(160, 160, 300, 300), (90, 100, 80, 70)], [(150, 170, 120, 100)]],
}


def _case(name, fam, hw, strides, nc, topk, boxes, what, dtypes=("fp32", "bf16"), seed=0, edit=None, gains=None, mode="default"):
    return dict(name=name, fam=fam, hw=hw, strides=strides, nc=nc, topk=topk, boxes=boxes, what=what, dtypes=dtypes, seed=seed, edit=edit,
                gains=gains, mode=mode)


S3 = (8.0, 16.0, 32.0)
PRIMES3D = dict(loss2d=0.2, cls=0.3, depth=0.5, offset3d=0.7, size3d=1.1, heading=1.3)
PRIMES2D = dict(box=0.7, cls=1.3, dfl=0.3)

# `seed` draws the head maps (the boxes are fixed): where it is not 0, seed 0 left a top-k decision of that case closer than MARGIN_FLOOR
# on the host (a near-tie of the INPUT, tests/test_loss_ref_host.py), and the next seed that clears it was taken.
CASES = [
    # ---- 3D: DDDetectionLoss ---------------------------------------------------------------------------------------------
    *[_case(f"l3_nc{nc}_k{k}", "3d", (320, 320), S3, nc, k, "normal", f"loss_kernel<T, {nc}> (Why 1): gr[nc + j], NC + 35 store loop, tscores[i * nc + c]")
      for nc in (1, 2, 4, 5) for k in (8, 1)],
    _case("l3_kitti", "3d", (384, 1280), S3, 3, 8, "kitti", "non-square maps 48x160 / 24x80 / 12x40: the hy = r / W walk (Why 4); wide-flat and tall-thin boxes"),
    _case("l3_nl1", "3d", (256, 256), (8.0,), 3, 8, "normal256", "nl = 1 in anchor_ptr / fill_levels (Why 4)"),
    _case("l3_nl2", "3d", (256, 256), (8.0, 16.0), 3, 8, "normal256", "nl = 2 (Why 4)"),
    _case("l3_nl4", "3d", (256, 256), (8.0, 16.0, 32.0, 64.0), 3, 8, "normal256", "nl = 4 = MAXL (Why 4)"),
    *[_case(f"l3_hires_k{k}", "3d", (1280, 1280), S3, 3, k, "hires", "A = 33600: the global-memory branch of topk_kernel, chosen[] skip list (Why 3)",
            dtypes=("fp32",)) for k in (8, 1)],
    _case("l3_empty_image", "3d", (320, 320), S3, 3, 8, "empty_image", "image 1 of 3 has no row: all background, dense cls gradient (Why 5)"),
    _case("l3_tiny", "3d", (320, 320), S3, 3, 8, "tiny", "a box with no anchor centre inside: all-zero metric row, every candidate dropped, pa/po stay 0 (Why 5)"),
    _case("l3_no_fg", "3d", (320, 320), S3, 3, 8, "no_fg", "boxes but no foreground: scal = [1, 0], inv2 = 1/0 never used (Why 5); the pinned divergence"),
    _case("l3_dup_nested", "3d", (320, 320), S3, 3, 8, "dup_nested", "duplicated and nested boxes: cnt > 1 of resolve_kernel, first maximum over exact ties (Why 5); "
          "seed 0: bf16 top-k gap of one box 2.3e-4, under the floor; seed 1: an anchor claimed by both duplicates whose keypoint similarities are the "
          "same real number (size-independent L1), equal on the host and one ulp apart on the device", seed=2),
    _case("l3_dup_box_only", "3d", (320, 320), S3, 3, 8, "dup_nested", "the same under box_only, where `second` is the CIoU: exact ties of duplicated rows",
          mode="box_only"),
    _case("l3_border", "3d", (320, 320), S3, 3, 8, "border", "boxes reaching over the image border (Why 5)"),
    _case("l3_capacity", "3d", (320, 320), S3, 3, 8, "capacity", "64 boxes in one image: n_used == n == TARGET_CAP (Why 5)", dtypes=("fp32",)),
    _case("l3_topk16", "3d", (320, 320), S3, 3, 16, "normal", "topk = 16, the kernel's upper bound: chosen[16] (Why 5)"),
    _case("l3_saturated", "3d", (320, 320), S3, 3, 8, "normal", "class and heading logits up to +-30: log1pf(expf(-|x|)), sigmoid_f, heading log-sum-exp (Why 6)",
          edit="saturate"),
    _case("l3_gain_zero", "3d", (320, 320), S3, 3, 8, "normal", "gain loss2d = 0: o2d / s2d gradients exactly 0 (Why 6)", gains=dict(loss2d=0.0)),
    _case("l3_gain_primes", "3d", (320, 320), S3, 3, 8, "normal", "six distinct gains (Why 6)", gains=PRIMES3D),
    _case("l3_kps_only_l2", "3d", (320, 320), S3, 3, 8, "normal", "assigner mode kps_only_l2, now with items and gradient", mode="kps_only_l2"),
    _case("l3_box_only", "3d", (320, 320), S3, 3, 8, "normal", "assigner mode box_only, now with items and gradient", mode="box_only"),
    _case("l3_dual_o2o", "3d", (320, 320), S3, 2, 1, "normal", "one-to-one half of the DualLoss3dFn case (nc = 2, no = 37: odd element offset) (Why 7)"),
    _case("l3_dual_o2m", "3d", (320, 320), S3, 2, 8, "normal", "one-to-many half of the DualLoss3dFn case (Why 7)", seed=1000),
    # ---- 2D: v8DetectionLoss -----------------------------------------------------------------------------------------------
    _case("l2_nc3_k10", "2d", (320, 320), S3, 3, 10, "normal", "loss2d_kernel<T, VEC = false> (Why 2): the KITTI 2D class count"),
    _case("l2_nc3_k1", "2d", (320, 320), S3, 3, 1, "normal", "scalar path, one-to-one top-k"),
    _case("l2_nc1", "2d", (320, 320), S3, 1, 10, "normal", "scalar path, nc = 1"),
    _case("l2_nc20", "2d", (320, 320), S3, 20, 10, "normal", "nc = 20: VEC in fp32 (20 % 4 == 0), scalar in bf16 (20 % 8 != 0)"),
    _case("l2_nc80_kitti", "2d", (384, 1280), S3, 80, 10, "kitti", "VEC path off the fixture, non-square maps (Why 4)"),
    _case("l2_nc8_kitti", "2d", (384, 1280), S3, 8, 10, "kitti", "VEC path with a single bf16 chunk of classes, non-square maps"),
    _case("l2_nl1", "2d", (256, 256), (8.0,), 3, 10, "normal256", "nl = 1 in fill2d (Why 4)"),
    _case("l2_nl2", "2d", (256, 256), (8.0, 16.0), 3, 10, "normal256", "nl = 2 (Why 4)"),
    _case("l2_nl4", "2d", (256, 256), (8.0, 16.0, 32.0, 64.0), 8, 10, "normal256", "nl = 4 = MAXL, VEC (Why 4)"),
    *[_case(f"l2_hires_k{k}", "2d", (1280, 1280), S3, 80, k, "hires", "A = 33600: global-memory top-k (Why 3) with the 2D metric", dtypes=("fp32",))
      for k in (10, 1)],
    _case("l2_dfl_clamp", "2d", (320, 320), S3, 3, 10, "big", "a 300 px box assigned to stride-8 anchors: DFL target clamped at reg_max - 1 - 0.01 (Why 6)",
          edit="dfl_clamp"),
    _case("l2_ciou_inside", "2d", (320, 320), S3, 3, 10, "normal", "predicted distances shrunk: prediction inside target (CIoU sub-gradients, Why 6)",
          edit=("tilt", -0.6)),
    _case("l2_ciou_outside", "2d", (320, 320), S3, 3, 10, "normal", "predicted distances stretched: target inside prediction (Why 6)", edit=("tilt", 0.6)),
    _case("l2_empty_image", "2d", (320, 320), S3, 3, 10, "empty_image", "image 1 of 3 has no row (Why 5)"),
    _case("l2_tiny", "2d", (320, 320), S3, 3, 10, "tiny", "a box with no anchor centre inside (Why 5)"),
    _case("l2_no_fg", "2d", (320, 320), S3, 3, 10, "no_fg", "boxes but no foreground: items [0, bce, 0] (Why 5)"),
    _case("l2_dup_nested", "2d", (320, 320), S3, 3, 10, "dup_nested", "duplicated and nested boxes: exact ties in resolve_kernel (Why 5)"),
    _case("l2_border", "2d", (320, 320), S3, 3, 10, "border", "boxes reaching over the image border (Why 5)"),
    _case("l2_capacity", "2d", (320, 320), S3, 3, 10, "capacity", "64 boxes in one image (Why 5)", dtypes=("fp32",)),
    _case("l2_topk16", "2d", (320, 320), S3, 3, 16, "normal", "topk = 16 with the 2D metric"),
    _case("l2_saturated", "2d", (320, 320), S3, 3, 10, "normal", "class logits up to +-30 (Why 6)", edit="saturate"),
    _case("l2_gain_zero", "2d", (320, 320), S3, 3, 10, "normal", "gain cls = 0: class gradient exactly 0, scalar path (Why 6)", gains=dict(cls=0.0)),
    _case("l2_gain_primes", "2d", (320, 320), S3, 3, 10, "normal", "three distinct gains, scalar path: a gain missing from a gradient shows (Why 6)",
          gains=PRIMES2D),
    _case("l2_gain_primes_vec", "2d", (320, 320), S3, 8, 10, "normal", "three distinct gains, VEC path", gains=PRIMES2D),
]
BY_NAME = {c["name"]: c for c in CASES}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def case_ids(fam=None):
    """[(case name, dtype name)] of the table, optionally of one family"""
    return [(c["name"], d) for c in CASES if fam in (None, c["fam"]) for d in c["dtypes"]]


def mean_sizes(nc):
    return torch.tensor([[v + 0.1 * (i // 3) for v in KITTI_MEAN[i % 3]] for i in range(nc)])


def level_shapes(hw, strides):
    return [(int(hw[0] // s), int(hw[1] // s)) for s in strides]


def make_batch(case):
    """the ground truth of a case; rows of the images are interleaved (image 0, 1, 2, 0, 1, ...) as a shuffled loader would leave them"""
    H, W = case["hw"]
    nc = case["nc"]
    per = BOXES[case["boxes"]]
    order = [(b, j) for j in range(max(len(p) for p in per)) for b in range(len(per)) if j < len(per[b])]
    n = len(order)
    g = torch.Generator().manual_seed(1234)
    px = torch.tensor([per[b][j] for b, j in order], dtype=torch.float32).view(n, 4)
    scale = torch.tensor([W, H, W, H], dtype=torch.float32)
    c2 = px[:, :2].clone()
    batch = {
        "batch_idx": torch.tensor([float(b) for b, _ in order]), "cls": (torch.arange(n) % nc).float().view(n, 1), "bboxes": px / scale,
        "center_2d": c2, "size_2d": px[:, 2:].clone(), "center_3d": c2 + 2.0 * torch.randn(n, 2, generator=g),
        "size_3d": 0.1 * torch.randn(n, 3, generator=g), "depth": 5 + 55 * torch.rand(n, generator=g),
        "heading_bin": torch.randint(0, 12, (n,), generator=g).float(), "heading_res": (torch.rand(n, generator=g) - 0.5) * (math.pi / 6),
        "calib": torch.tensor([[W / 2, H / 2, 700.0, 700.0, 0.06, -0.002]]).repeat(len(per), 1), "mean_sizes": mean_sizes(nc),
    }
    for i, (b, j) in enumerate(order):  # a duplicated box is the same row twice, label apart
        for i0, (b0, j0) in enumerate(order[:i]):
            if b0 == b and per[b0][j0] == per[b][j]:
                for k in ("center_3d", "size_3d", "depth", "heading_bin", "heading_res"):
                    batch[k][i] = batch[k][i0]
                break
    return batch, len(per)


def make_maps(case, dtype=torch.float32, seed=None):
    """head maps drawn as the existing loss tests draw them (3D: class logits shifted down, positive sizes, depth 10..40; 2D: plain
    normal logits), edited where the case says so, rounded to `dtype` and returned as fp32 (B, no, H, W) host tensors"""
    nc, fam = case["nc"], case["fam"]
    B = len(BOXES[case["boxes"]])
    g = torch.Generator().manual_seed(case["seed"] if seed is None else seed)
    no = nc + 35 if fam == "3d" else nc + 64
    maps = []
    for lvl, (h, w) in enumerate(level_shapes(case["hw"], case["strides"])):
        t = torch.randn(B, no, h, w, generator=g)
        if fam == "3d":
            t[:, :nc] -= 2.0
            t[:, nc + 2:nc + 4] = 2 + 4 * torch.rand(B, 2, h, w, generator=g)
            t[:, nc + 33] = 10 + 30 * torch.rand(B, h, w, generator=g)
        edit = case["edit"]
        cls = slice(0, nc) if fam == "3d" else slice(64, 64 + nc)
        if edit == "saturate":
            t[:, cls] *= 30.0 / t[:, cls].abs().max()
            if fam == "3d":
                hb = slice(nc + 9, nc + 21)
                t[:, hb] *= 30.0 / t[:, hb].abs().max()
        elif edit == "dfl_clamp" and lvl == 0:
            # the 300 px box is row 0 of image 0 (label 0), centred at (160, 160): stride-8 cells 17..22 get a strong class-0 logit and
            # long predicted distances, so the top-k of that box lands on them although they are > 15 cells from its sides
            t[0, 64, 17:23, 17:23] += 6.0
            t[0, :64, 17:23, 17:23].view(4, 16, 6, 6)[:, 15] += 8.0
        elif isinstance(edit, tuple) and edit[0] == "tilt":
            t[:, :64] += (edit[1] * torch.arange(16.0)).repeat(4).view(1, 64, 1, 1)
        maps.append(t.to(dtype).float())
    return maps


def hyp_of(case):
    h = dict(RS.HYP)
    h.update(case["gains"] or {})
    return h


def flatten(maps):
    B, no = maps[0].shape[:2]
    return torch.cat([m.reshape(B, no, -1) for m in maps], 2).permute(0, 2, 1)


def anchors(shapes, strides, dtype=torch.float32):
    anc, st = RS.make_anchors(shapes, strides)
    return anc.to(dtype), st.to(dtype)


def rows_of(batch, fam):
    if fam == "3d":
        keys = ("batch_idx", "cls", "bboxes", "center_2d", "size_2d", "center_3d", "size_3d", "depth", "heading_bin", "heading_res")
    else:
        keys = ("batch_idx", "cls", "bboxes")
    return torch.cat([batch[k].float().view(batch[k].shape[0], -1) for k in keys], 1)


# ---------------------------------------------------------------------------------------------------------
# assignment: the oracle's, plus its metrics for the margin check
# ---------------------------------------------------------------------------------------------------------
def metrics3d(cat, gpad, calib, msz, shapes, strides, nc, hyp, mode, dtype=torch.float32):
    """(align, second, gmask) of restate.tal3d (:736-763), in `dtype`.  The discrete choices inside (arg-max class for the mean size,
    arg-max heading bin) are taken from the fp32 values, as the oracle takes them, also when dtype is float64."""
    amax = cat[..., :nc].float().sigmoid().argmax(-1)
    cat, gpad, calib, msz = cat.to(dtype), gpad.to(dtype), calib.to(dtype), msz.to(dtype)
    sc, o2d, s2d, o3d, s3d, hd, dep, dun = cat.split((nc, 2, 2, 2, 3, 24, 1, 1), -1)
    anc, st = anchors(shapes, strides, dtype)
    gl, gb, gc2, gs2, gc3, gs3, gd, ghb, ghr = gpad.split((1, 4, 2, 2, 2, 3, 1, 1, 1), 2)
    mask_gt = (gb.sum(2, keepdim=True) > 0).to(dtype)
    cen = anc + o2d
    pb = torch.cat((cen - s2d / 2, cen + s2d / 2), -1) * st
    A = cat.shape[1]
    pc3 = anc * st + o3d * st
    ps3 = msz[amax] + s3d
    lab = gl.squeeze(-1).long()
    g_kps = RS.keypoints_3d(gc3, gd, msz[lab.clamp(min=0)] + gs3, ghb, ghr, calib)
    p_kps = RS.keypoints_3d(pc3, dep, ps3, hd[..., :12], hd[..., 12:], calib)
    in_g = RS._in_gts(anc * st, gb)
    gmask = in_g * mask_gt if mode["constrain_anchors"] else mask_gt.expand(-1, -1, A)
    m = gmask.bool()
    s = sc.sigmoid().gather(2, lab.clamp(min=0)[:, None, :].expand(-1, A, -1)).permute(0, 2, 1)
    s = torch.where(m, s, torch.zeros_like(s))
    diff = p_kps[:, None] - g_kps[:, :, None]
    if mode["kps_dist_metric"] == "l1":
        sim_all = 1 / torch.exp(diff.abs().sum((-1, -2)) / 24)
    else:
        sim_all = 1 / torch.exp(0.5 * (diff * diff).sum((-1, -2)) / 24)
    sim = torch.where(m, sim_all, torch.zeros_like(sim_all))
    ov = torch.where(m, RS.ciou(gb[:, :, None, :], pb[:, None, :, :]).clamp(min=0), torch.zeros_like(sim_all))
    a, b, c = hyp["tal_alpha"], hyp["tal_beta"], hyp["tal_gamma"]
    if mode["tal_2d"] and mode["tal_3d"]:
        return s.pow(a) * ov.pow(b) * sim.pow(c), sim, gmask, mask_gt
    if mode["tal_3d"]:
        return s.pow(a) * sim.pow(c), sim, gmask, mask_gt
    return s.pow(a) * ov.pow(b), ov, gmask, mask_gt


def metrics2d(cat, gpad, shapes, strides, nc, dtype=torch.float32, alpha=0.5, beta=6.0):
    """(align, overlaps, gmask, mask_gt) of restate.tal2d (:705-712), in `dtype`"""
    cat, gpad = cat.to(dtype), gpad.to(dtype)
    dist, sc = cat.split((64, nc), -1)
    B, A = cat.shape[:2]
    anc, st = anchors(shapes, strides, dtype)
    gl, gb = gpad.split((1, 4), 2)
    mask_gt = (gb.sum(2, keepdim=True) > 0).to(dtype)
    d = dist.view(B, A, 4, 16).softmax(3).matmul(torch.arange(16, dtype=dtype))
    pb = torch.cat((anc - d[..., :2], anc + d[..., 2:]), -1) * st
    in_g = RS._in_gts(anc * st, gb)
    gmask = in_g * mask_gt
    m = gmask.bool()
    lab = gl.squeeze(-1).long()
    s = sc.sigmoid().gather(2, lab.clamp(min=0)[:, None, :].expand(-1, A, -1)).permute(0, 2, 1)
    s = torch.where(m, s, torch.zeros_like(s))
    ov = RS.ciou(gb[:, :, None, :], pb[:, None, :, :]).clamp(min=0)
    ov = torch.where(m, ov, torch.zeros_like(ov))
    return s.pow(alpha) * ov.pow(beta), ov, gmask, mask_gt


def replay(align, second, gmask, mask_gt, topk):
    """fg_mask, target_gt_idx and the multiplicity of every anchor from the metrics, by the oracle's own top-k and conflict rules"""
    mask_pos = RS.stable_topk_mask(align, topk, mask_gt) * gmask
    multi = mask_pos.sum(-2)
    gt_idx, fg, _ = RS._resolve(mask_pos, second)
    return fg.bool(), gt_idx, multi


def assign(case, maps, batch, B):
    """the oracle's assignment of a case: dict(fg, gt_idx, t_sc, gpad, align, second, gmask, mask_gt, multi, twins), all fp32 / integer"""
    fam, nc, topk = case["fam"], case["nc"], case["topk"]
    H, W = case["hw"]
    strides = list(case["strides"])
    shapes = level_shapes(case["hw"], strides)
    cat = flatten(maps)
    anc, st = anchors(shapes, strides)
    scale = torch.tensor([W, H, W, H], dtype=torch.float32)
    hyp, mode = hyp_of(case), MODES[case["mode"]]
    if fam == "3d":
        gpad = RS.pad_targets(rows_of(batch, "3d"), B, 17, scale)
        sc, o2d, s2d, o3d, s3d, hd, dep, dun = cat.split((nc, 2, 2, 2, 3, 24, 1, 1), -1)
        gts = gpad.split((1, 4, 2, 2, 2, 3, 1, 1, 1), 2)
        mask_gt = (gts[1].sum(2, keepdim=True) > 0).float()
        cen = anc + o2d
        pb = torch.cat((cen - s2d / 2, cen + s2d / 2), -1) * st
        targets, fg, gt_idx = RS.tal3d(sc.sigmoid(), pb, torch.cat((o3d, s3d, hd, dep, dun), -1), anc * st, gts, mask_gt, st, batch["calib"].float(),
                                       batch["mean_sizes"].float(), topk, nc, hyp["tal_alpha"], hyp["tal_beta"], hyp["tal_gamma"],
                                       use_2d=mode["tal_2d"], use_3d=mode["tal_3d"], kps_dist=mode["kps_dist_metric"], constrain=mode["constrain_anchors"])
        t_sc = targets[1]
        align, second, gmask, mask_gt = metrics3d(cat, gpad, batch["calib"], batch["mean_sizes"], shapes, strides, nc, hyp, mode)
    else:
        gpad = RS.pad_targets(rows_of(batch, "2d"), B, 5, scale)
        dist, sc = cat.split((64, nc), -1)
        gl, gb = gpad.split((1, 4), 2)
        mask_gt = (gb.sum(2, keepdim=True) > 0).float()
        d = dist.view(B, -1, 4, 16).softmax(3).matmul(torch.arange(16, dtype=torch.float32))
        pb = torch.cat((anc - d[..., :2], anc + d[..., 2:]), -1)
        _, _, t_sc, fg, gt_idx = RS.tal2d(sc.sigmoid(), pb * st, anc * st, gl, gb, mask_gt, topk, nc)
        align, second, gmask, mask_gt = metrics2d(cat, gpad, shapes, strides, nc)
    _, _, multi = replay(align, second, gmask, mask_gt, topk)
    return dict(fg=fg, gt_idx=gt_idx, t_sc=t_sc, gpad=gpad, align=align, second=second, gmask=gmask, mask_gt=mask_gt, multi=multi,
                twins=twin_boxes(case, gpad, batch.get("mean_sizes")))


def _decisions(align, second, mask_gt, topk, gmask):
    """the entries a decision hangs on: per valid box with more than k non-zero metrics its k-th and (k+1)-th largest (hi, lo, index
    pairs), per multiply-selected anchor the two largest entries of its `second` column"""
    if gmask is None:
        gmask = ((second > 0) | (align > 0)).to(align.dtype)
    B, n, A = align.shape
    srt, idx = torch.sort(align, dim=-1, descending=True, stable=True)
    nz = (align > 0).sum(-1)
    rows = (mask_gt.view(B, n) > 0) & (nz > topk)
    k = min(topk, A - 1)
    hi, lo = srt[..., k - 1][rows], srt[..., k][rows]
    mask_pos = RS.stable_topk_mask(align, topk, mask_gt) * gmask
    cols = mask_pos.sum(-2) > 1  # (B, A)
    top2 = second.permute(0, 2, 1)[cols].topk(min(2, n), -1)[0] if n > 1 else second.new_zeros(0, 2)
    return (hi, lo, rows, idx[..., :k + 1]), (top2, cols)


def assignment_margin(align, second, mask_gt, topk, gmask=None, twins=None):
    """How far the assignment is from flipping, from the oracle's tensors alone (align, second: (B, n, A); mask_gt (B, n, 1)):
    (a) per valid box with more than k non-zero metrics, the relative gap (m_k - m_k+1) / m_k between its k-th and (k+1)-th largest
        non-zero metric; (b) per anchor that more than one box selected, the relative gap between the two largest entries of `second`
    over the boxes of its image.  Entries that are EXACTLY equal by construction (duplicated boxes; zero metrics, which (a) never looks
    at) are left out: the tie rule (lowest index in the top-k, first maximum in the conflict resolution) decides them identically
    everywhere.  `gmask` (B, n, A): the candidate mask of the assigner (anchors inside the box); default: where a metric is non-zero.
    `twins` (B, n, n) bool: the pairs of boxes whose `second` is the same computation on the same numbers; default: every equality counts
    as deliberate.  With it, an equality between other boxes is a near-tie of gap 0: the L1 keypoint distance to two boxes that differ in
    size alone is the same real number wherever the predicted corners lie outside both, and rounding decides which comes out larger.
    -> (gaps_a, gaps_b, n_exact_ties_b), 1-D tensors"""
    (hi_v, lo_v, rows, idx), (top2, cols) = _decisions(align, second, mask_gt, topk, gmask)
    gaps_a = (hi_v - lo_v) / hi_v
    if top2.numel():
        tie = top2[:, 0] == top2[:, 1]
        if twins is not None:
            i2 = second.permute(0, 2, 1)[cols].topk(2, -1)[1]
            b = cols.nonzero()[:, 0]
            tie = tie & twins[b, i2[:, 0], i2[:, 1]]
        gaps_b = ((top2[:, 0] - top2[:, 1]) / top2[:, 0])[~tie]
        ties = int(tie.sum())
    else:
        gaps_b, ties = align.new_zeros(0), 0
    return gaps_a, gaps_b, ties


def twin_boxes(case, gpad, msz=None):
    """(B, n, n) bool: pairs of rows whose conflict-resolution metric is the same computation on the same numbers: equal boxes where it is
    the CIoU (2D, box_only); rows equal in everything but a label that selects an equal mean size where it is the keypoint similarity"""
    if case["fam"] == "2d" or not MODES[case["mode"]]["tal_3d"]:
        key = gpad[..., 1:5]
    else:
        key = torch.cat((gpad[..., 1:], msz[gpad[..., 0].long().clamp(min=0)]), -1)
    return (key[:, :, None, :] == key[:, None, :, :]).all(-1)


def metrics64(case, maps, batch, a):
    """(align, second) of a case in float64, for `metric_rounding`"""
    shapes, strides = level_shapes(case["hw"], case["strides"]), list(case["strides"])
    cat = flatten(maps)
    if case["fam"] == "3d":
        r = metrics3d(cat, a["gpad"], batch["calib"], batch["mean_sizes"], shapes, strides, case["nc"], hyp_of(case), MODES[case["mode"]], torch.float64)
    else:
        r = metrics2d(cat, a["gpad"], shapes, strides, case["nc"], torch.float64)
    return r[0], r[1]


def metric_rounding(a32, s32, a64, s64, mask_gt, topk, gmask):
    """largest relative difference between the fp32 and the float64 metrics over the entries `assignment_margin` looks at"""
    (_, _, rows, idx), (_, cols) = _decisions(a32, s32, mask_gt, topk, gmask)
    worst = 0.0
    if rows.any():
        x, y = a32.gather(-1, idx)[rows].double(), a64.gather(-1, idx)[rows]
        worst = max(worst, float(((x - y).abs() / y.abs().clamp(min=1e-300)).max()))
    if cols.any():
        x, y = s32.permute(0, 2, 1)[cols].double(), s64.permute(0, 2, 1)[cols]
        top = y >= y.topk(min(2, y.shape[-1]), -1)[0][:, -1:]
        worst = max(worst, float((((x - y).abs() / y.abs().clamp(min=1e-300)))[top].max()))
    return worst


# ---------------------------------------------------------------------------------------------------------
# loss terms in float64, the assignment given
# ---------------------------------------------------------------------------------------------------------
def _take(gt, gt_idx):
    B, A = gt_idx.shape
    return gt[torch.arange(B)[:, None].expand(B, A), gt_idx]  # (B, A, width)


def loss3d_terms(cat, assignment, gt, strides, shapes, gains):
    """The six items of utils/loss.py:821-963 (+ :1112-1136) as `restate.loss3d_one` states them, in float64.
    cat (B, A, nc + 35) float64 (a function of leaves that require grad); assignment = (fg (B, A) bool, gt_idx (B, A) int64,
    target_scores (B, A, nc)); gt (B, n, 17) padded targets in pixels; gains: dict over GAINS3D.  -> items (6,) float64.

    One deliberate difference: with boxes but NO foreground anchor the upstream loss (and `restate.loss3d_one`) takes the "mean" L1 of
    empty tensors and returns NaN in items 0 (2D box) and 3 (3D offset); the HIP kernel returns 0 there, and so does this function
    (every foreground term is 0 when `fg` is empty).  DESIGN.md, Parity; pinned by tests/test_loss_ref_host.py."""
    fg, gt_idx, t_sc = assignment
    nc = cat.shape[-1] - 35
    dt = cat.dtype
    t_sc, gt = t_sc.to(dt), gt.to(dt)
    sc, o2d, s2d, o3d, s3d, hd, dep, dun = cat.split((nc, 2, 2, 2, 3, 24, 1, 1), -1)
    anc, st = anchors(shapes, strides, dt)
    anc_px = anc * st
    tss = t_sc.sum().clamp(min=1)
    w = [gains[k] for k in GAINS3D]
    items = [cat.new_zeros(()) for _ in range(6)]
    items[1] = F.binary_cross_entropy_with_logits(sc, t_sc, reduction="none").sum() / tss * w[1]
    if fg.any():
        g = _take(gt, gt_idx)[fg]  # (nfg, 17): cls | box | c2 | s2 | c3 | s3 | depth | hbin | hres
        apx = anc_px.expand(cat.shape[0], -1, -1)[fg]
        off_l = F.l1_loss((o2d * st)[fg], g[:, 5:7] - apx, reduction="mean")
        siz_l = F.l1_loss((s2d * st)[fg], g[:, 7:9], reduction="mean")
        items[0] = (siz_l + off_l) / tss * w[0]
        pd, pu = dep[fg].squeeze(-1), dun[fg].squeeze(-1)
        items[2] = (1.4142 * torch.exp(-0.5 * pu) * (pd - g[:, 14]).abs() + 0.5 * pu).sum() / tss * w[2]
        items[3] = F.l1_loss((o3d * st)[fg], g[:, 9:11] - apx, reduction="mean") / tss * w[3]
        items[4] = F.l1_loss(s3d[fg], g[:, 11:14], reduction="sum") / tss * w[4]
        ph = hd[fg]
        tb = g[:, 15].long()
        ce = F.cross_entropy(ph[:, :12], tb, reduction="sum")
        reg = F.l1_loss(ph[:, 12:].gather(1, tb.view(-1, 1)).squeeze(1), g[:, 16], reduction="sum")
        items[5] = (ce + reg) / tss * w[5]
    return torch.stack(items)


def loss2d_terms(cat, assignment, gt, strides, shapes, gains):
    """The three items (box, cls, dfl) of utils/loss.py:206-257 (+ BboxLoss :82-113) as `restate.loss2d_one` states them, in float64.
    cat (B, A, 64 + nc); assignment as in `loss3d_terms`; gt (B, n, 5) = cls | box xyxy px; gains: dict over GAINS2D."""
    fg, gt_idx, t_sc = assignment
    nc = cat.shape[-1] - 64
    dt = cat.dtype
    t_sc, gt = t_sc.to(dt), gt.to(dt)
    dist, sc = cat.split((64, nc), -1)
    B, A = cat.shape[:2]
    anc, st = anchors(shapes, strides, dt)
    d = dist.view(B, A, 4, 16).softmax(3).matmul(torch.arange(16, dtype=dt))
    pb = torch.cat((anc - d[..., :2], anc + d[..., 2:]), -1)
    tss = t_sc.sum().clamp(min=1)
    items = [cat.new_zeros(()) for _ in range(3)]
    items[1] = F.binary_cross_entropy_with_logits(sc, t_sc, reduction="none").sum() / tss
    if fg.any():
        t_box = _take(gt, gt_idx)[..., 1:5] / st
        wt = t_sc.sum(-1)[fg].unsqueeze(-1)
        iou = RS.ciou(pb[fg], t_box[fg]).unsqueeze(-1)
        items[0] = ((1.0 - iou) * wt).sum() / tss
        ltrb = torch.cat((anc - t_box[..., :2], t_box[..., 2:] - anc), -1).clamp(0, 15 - 0.01)[fg]
        pdist = dist[fg].view(-1, 16)
        tl = ltrb.long()
        tr = tl + 1
        wl = tr - ltrb
        wr = 1 - wl
        dfl = (F.cross_entropy(pdist, tl.view(-1), reduction="none").view(tl.shape) * wl +
               F.cross_entropy(pdist, tr.view(-1), reduction="none").view(tl.shape) * wr).mean(-1, keepdim=True)
        items[2] = (dfl * wt).sum() / tss
    return torch.stack(items) * torch.tensor([gains[k] for k in GAINS2D], dtype=dt)


def group_errors(grads, refs, groups):
    """per level and channel group: (max |grad - ref| / max(largest |ref| of the group in that level, 1e-6 x the largest |ref| of the whole
    map), index (b, c, y, x) of the worst element).  grads / refs: lists of (B, no, H, W); groups: [(name, width)] along the channel axis"""
    top = max(float(r.abs().max()) for r in refs)
    out = {}
    for lvl, (g, r) in enumerate(zip(grads, refs)):
        c0 = 0
        for name, width in groups:
            gs, rs = g[:, c0:c0 + width].double(), r[:, c0:c0 + width].double()
            d = (gs - rs).abs()
            den = max(float(rs.abs().max()), 1e-6 * top, 1e-300)
            b, c, hy, hx = [int(v) for v in torch.unravel_index(d.argmax(), d.shape)]
            out[(lvl, name)] = (float(d.max()) / den, (b, c0 + c, hy, hx))
            c0 += width
    return out


def reference(case, maps, assignment, gpad):
    """float64 items and d(sum of items)/d(map) per level of a case, on the given (fp32-valued) maps and assignment"""
    leaves = [m.double().requires_grad_(True) for m in maps]
    strides = list(case["strides"])
    fn = loss3d_terms if case["fam"] == "3d" else loss2d_terms
    items = fn(flatten(leaves), assignment, gpad, strides, level_shapes(case["hw"], strides), hyp_of(case))
    items.sum().backward()
    return items.detach(), [x.grad if x.grad is not None else torch.zeros_like(x) for x in leaves]


def restate_run(case, maps, batch):
    """restate.loss3d_one / loss2d_one on a default-mode case -> (items fp32, [gradient of sum(items) per level], aux)"""
    leaves = [m.clone().requires_grad_(True) for m in maps]
    fn = RS.loss3d_one if case["fam"] == "3d" else RS.loss2d_one
    loss, items, aux = fn(leaves, batch, list(case["strides"]), case["nc"], case["topk"], hyp_of(case))
    B = maps[0].shape[0]
    loss.backward()
    return items.detach(), [x.grad / B for x in leaves], aux


def model_of(case, **over):
    """the stand-in for a model that the product's loss classes take: head geometry + hyper-parameters"""
    nc, fam = case["nc"], case["fam"]
    head = SimpleNamespace(stride=torch.tensor(list(case["strides"])), nc=nc, no=nc + 35 if fam == "3d" else nc + 64, reg_max=16)
    hyp = dict(RS.HYP, distillation=False, fgdm_loss=False, fgdm_supervision=False, htl=False, **MODES[case["mode"]])
    hyp.update(case["gains"] or {})
    hyp.update(over)
    return SimpleNamespace(model=[head], args=SimpleNamespace(**hyp))
