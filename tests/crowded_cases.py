"""TEST INFRASTRUCTURE - the cases of the crowded 2D route (more than 64 boxes per image, `max_boxes`), shared by
tests/test_hip_losses_crowded.py (device) and tests/test_crowded_host.py (host).  Plain torch; never imports the HIP library.

The cases are dicts of the shape tests/loss_ref.py gives its own, so its batch / map / oracle / float64 functions take them as they
are; their boxes come from `crowd(count, ...)` and are registered in `loss_ref.BOXES` only while `registered()` is open.

A crowd is drawn once from a fixed generator and then salted with the shapes the assigner treats apart:
* every 9th box repeats the box five places before it (equal rows: exact ties in the conflict resolution, first maximum wins);
* every 13th box is 2 x 2 px around a point no anchor centre of stride 8 / 16 / 32 comes near (no candidate at all, normalisers stay 0);
* every 17th box hangs over the image border.
With several hundred boxes over 420 anchors most anchors are claimed more than once, so the arg-max over all rows and the per-box
normalisers decide the result.

`seeds` draws the head maps per dtype: the first seed at which every decision of the case clears `loss_ref.MARGIN_FLOOR` on the oracle's own
metrics (tests/test_crowded_host.py asserts that here, tests/test_hip_losses_crowded.py again before it looks at the device).
"""
import contextlib
from unittest import mock

import torch

import loss_ref as LR


def crowd(count, hw, seed, wh=(6.0, 56.0)):
    """`count` boxes (cx, cy, w, h) in pixels on an image of hw = (H, W)"""
    H, W = hw
    g = torch.Generator().manual_seed(seed)
    cx = (torch.rand(count, generator=g) * W).tolist()
    cy = (torch.rand(count, generator=g) * H).tolist()
    w = (wh[0] + (wh[1] - wh[0]) * torch.rand(count, generator=g)).tolist()
    h = (wh[0] + (wh[1] - wh[0]) * torch.rand(count, generator=g)).tolist()
    boxes = []
    for i in range(count):
        if i % 9 == 8:
            boxes.append(boxes[i - 5])
        elif i % 13 == 12:
            boxes.append((16.0 * (1 + i % (W // 16 - 1)) + 2.0, 16.0 * (1 + (i // 7) % (H // 16 - 1)) + 2.0, 2.0, 2.0))
        elif i % 17 == 16:
            side = (i // 17) % 4
            boxes.append(((3.0, W - 2.0, cx[i], cx[i])[side], (cy[i], cy[i], 2.0, H - 3.0)[side], round(w[i]) + 8.0, round(h[i]) + 8.0))
        else:
            boxes.append((round(cx[i], 1), round(cy[i], 1), round(w[i], 1), round(h[i], 1)))
    return boxes


SMALL = (128, 160)  # 16 x 20 + 8 x 10 + 4 x 5 = 420 anchors
BOXES = {
    "crowd65": [crowd(65, SMALL, 1), []],
    "crowd129": [crowd(129, SMALL, 2), crowd(3, SMALL, 3)],
    "crowd512": [crowd(512, SMALL, 4), crowd(70, SMALL, 5)],
    "crowd70_640": [crowd(70, (640, 640), 6, wh=(20.0, 300.0))],
    "crowd65_1280": [crowd(65, (1280, 1280), 7, wh=(40.0, 500.0))],
    "crowd10": [crowd(10, (320, 320), 8, wh=(30.0, 150.0)), crowd(4, (320, 320), 9, wh=(30.0, 150.0))],
    "crowd100": [crowd(100, SMALL, 10), crowd(3, SMALL, 11)],
}


def _case(name, hw, nc, topk, boxes, what, seeds, max_boxes=128):
    return dict(name=name, fam="2d", hw=hw, strides=LR.S3, nc=nc, topk=topk, boxes=boxes, what=what, dtypes=tuple(seeds), seed=None, seeds=seeds,
                edit=None, gains=None, mode="default", max_boxes=max_boxes)


CASES = [
    *[_case(f"c65_nc{nc}_k{k}", SMALL, nc, k, "crowd65", "65 boxes in image 0, none in image 1: one row past the dense route's capacity", SEEDS)
      for nc, k, SEEDS in ((1, 10, dict(fp32=1, bf16=1)), (1, 1, dict(fp32=0, bf16=0)), (80, 10, dict(fp32=1, bf16=1)), (80, 1, dict(fp32=0, bf16=0)))],
    _case("c129", SMALL, 3, 10, "crowd129", "129 boxes over 420 anchors: most anchors multiply claimed", dict(fp32=0, bf16=0), max_boxes=192),
    _case("c512_k10", SMALL, 80, 10, "crowd512", "512 boxes = the largest capacity, 70 in the other image", dict(fp32=1, bf16=1), max_boxes=512),
    _case("c512_k1", SMALL, 3, 1, "crowd512", "512 boxes, one-to-one top-k", dict(fp32=0), max_boxes=512),
    _case("c70_lds", (640, 640), 3, 10, "crowd70_640", "A = 8400: the cells' metrics stay in LDS", dict(fp32=0)),
    _case("c65_global", (1280, 1280), 3, 10, "crowd65_1280", "A = 33600: the metric row does not fit LDS, every pass forms it again", dict(fp32=0)),
]
BY_NAME = {c["name"]: c for c in CASES}
# the batches both routes take (max_boxes=None against max_boxes=128): 10 boxes, and loss_ref's own 64-box grid
BOTH_ROUTES = [
    _case("r10", (320, 320), 3, 10, "crowd10", "10 + 4 boxes through both routes", dict(fp32=0, bf16=1)),
    _case("r64", (320, 320), 3, 10, "capacity", "64 boxes (loss_ref's capacity grid) through both routes", dict(fp32=0)),
]


def case_ids(cases=CASES):
    return [(c["name"], d) for c in cases for d in c["dtypes"]]


@contextlib.contextmanager
def registered():
    """the crowds visible to loss_ref.make_batch / make_maps, which look their boxes up by name"""
    with mock.patch.dict(LR.BOXES, BOXES):
        yield


def build(case, dname):
    """-> (batch, B, maps, oracle assignment) of a case in one dtype"""
    with registered():
        batch, B = LR.make_batch(case)
        maps = LR.make_maps(case, LR.DTYPES[dname], seed=case["seeds"][dname])
        a = LR.assign(case, maps, batch, B)
    return batch, B, maps, a


def margins(case, a):
    """(smallest top-k gap, smallest conflict gap, exact ties) of a case's oracle assignment"""
    ga, gb, ties = LR.assignment_margin(a["align"], a["second"], a["mask_gt"], case["topk"], a["gmask"], a["twins"])
    return (float(ga.min()) if ga.numel() else float("inf")), (float(gb.min()) if gb.numel() else float("inf")), ties
