"""CPU: the float64 restatement of the feature-distillation item (tests/distill_ref.py) against the reference's own
`SupervisionLoss.forward_head` (tests/golden/distill.npz, tools/make_golden_distill.py), and the host-side surface of the feature."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import distill_ref as DR
import yolov10_3d_amd as y3d
from yolov10_3d_amd import ddp, loss as PL


def fixture():
    return np.load(os.path.join(GOLDEN, "distill.npz"))


def cases(z):
    return sorted(k[:-4] for k in z.files if k.endswith("/cfg"))


def run_case(z, name):
    C, crit, T, nomix = z[f"{name}/cfg"]
    i = {k: z[f"in{int(C)}/{k}"] for k in ("emb", "teacher", "gt_center", "mask_gt", "fg", "gt_idx", "mixed")}
    return DR.forward_head(i["emb"], i["teacher"], i["gt_center"], i["mask_gt"], i["fg"], i["gt_idx"], i["mixed"], tuple(z["img_wh"]), T,
                           float(z["weight"]), DR.CRITERIA[int(crit)], bool(nomix)), i


def test_fixture_covers_the_cases_the_feature_names():
    z = fixture()
    cfg = np.stack([z[f"{n}/cfg"] for n in cases(z)])
    assert set(cfg[:, 0]) == {64.0, 128.0} and set(cfg[:, 1]) == {0.0, 1.0, 2.0} and set(cfg[:, 2]) == {1.0, 2.0} and set(cfg[:, 3]) == {0.0, 1.0}
    for C in (64, 128):
        m, fg = z[f"in{C}/mask_gt"], z[f"in{C}/fg"]
        assert z[f"in{C}/mixed"].tolist() == [True, False, False, False]
        assert not m[2].any() and not fg[2].any(), "image 2 has no object"
        assert all(fg[b].any() for b in (0, 1, 3)), "the reference is NaN for an image with objects and no foreground anchor"
        h, w = z[f"in{C}/teacher"].shape[2:]
        assert h != w and (h, w) not in {tuple(l) for l in z["levels"]}
        assert z[f"in{C}/emb"].shape[2] == int(np.prod(z["levels"], 1).sum()) and len(z["levels"]) == 3


def test_restatement_gradients_match_the_reference():
    z = fixture()
    for name in cases(z):
        (loss, grad, rows), i = run_case(z, name)
        ref = z[f"{name}/grad"]
        err = np.abs(grad - ref).max() / np.abs(ref).max()
        print(f"{name}: gradient max-norm relative error {err:.3e}")
        assert err <= 1e-10, f"{name}: {err:.3e}"
        part = [b for b in range(4) if i["mask_gt"][b].any() and not (z[f"{name}/cfg"][3] and i["mixed"][b])]
        assert set(rows) == {(b, a) for b in part for a in np.nonzero(i["fg"][b])[0]}


def test_restatement_loss_matches_the_reference():
    z = fixture()
    for name in cases(z):
        (loss, _, _), _ = run_case(z, name)
        ref = float(z[f"{name}/loss"])
        print(f"{name}: loss {loss:.9f} reference {ref:.9f}")
        assert abs(loss - ref) <= 1e-6 * abs(ref)  # the reference keeps each image's loss in a float32 tensor


def test_teacher_pixels_are_the_references():
    z = fixture()
    for C in (64, 128):
        gtc, gi, fg, pix = z[f"in{C}/gt_center"], z[f"in{C}/gt_idx"], z[f"in{C}/fg"], z[f"in{C}/pix"]
        h, w = z[f"in{C}/teacher"].shape[2:]
        own = DR.teacher_pixels(gtc, tuple(z["img_wh"]), (w, h))
        for b in range(gtc.shape[0]):
            a = np.nonzero(fg[b])[0]
            assert np.array_equal(own[b][gi[b, a]], pix[b, a]), f"image {b}"
        # image 3: centres on .5 pixels round to the even neighbour, centres outside the image are clamped
        assert own[3].tolist() == [[2, 2], [2, 2], [0, 5], [15, 0]]


def test_no_foreground_rule_of_the_restatement():
    """an image with objects but no foreground anchor contributes 0 (the reference: NaN); every other image is unchanged"""
    z = fixture()
    name = "soft_t2_mix_c64"
    (l0, g0, _), i = run_case(z, name)
    fg = i["fg"].copy()
    fg[1] = False
    l1, g1, rows = DR.forward_head(i["emb"], i["teacher"], i["gt_center"], i["mask_gt"], fg, i["gt_idx"], i["mixed"], tuple(z["img_wh"]), 2.0,
                                   float(z["weight"]), "soft", False)
    assert np.isfinite(l1) and l1 < l0 and not g1[1].any() and np.array_equal(g1[[0, 2, 3]], g0[[0, 2, 3]]) and all(b != 1 for b, _ in rows)


def test_header_declares_the_distillation_entry_points():
    src = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "y3d.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+y3d_distill_loss\s*\(", src) and re.search(r"\bint\s+y3d_distill_scatter\s*\(", src)


def test_host_surface():
    hyp = dict(y3d.tasks.DEFAULT_HYP)
    assert hyp["distillation"] is False and (hyp["distillation_temp"], hyp["distillation_weight"], hyp["distillation_loss"], hyp["distillation_no_mixup"]) == (2, 0.75, "soft", True)
    assert "teacher_emb" in ddp.PER_IMAGE_KEYS
    off, on = SimpleNamespace(**hyp), SimpleNamespace(**dict(hyp, distillation=True))
    assert PL.loss_names(off) == ["box_om", "cls_om", "dep_om", "o3d_om", "s3d_om", "hd_om", "box_oo", "cls_oo", "dep_oo", "o3d_oo", "s3d_oo", "hd_oo"]
    assert PL.loss_names(on) == ["box_om", "cls_om", "dep_om", "o3d_om", "s3d_om", "hd_om", "dis_om", "box_oo", "cls_oo", "dep_oo", "o3d_oo", "s3d_oo", "hd_oo", "dis_oo"]
    head = SimpleNamespace(stride=torch.tensor([8.0, 16.0, 32.0]), nc=3, no=38)
    crit = PL.DetectLoss3d(SimpleNamespace(model=[head], args=on))  # constructing it with the switch on no longer raises
    assert crit.one2one.distillation and head.distill is True
    with pytest.raises(RuntimeError, match="Unknown criterion"):
        PL.DDDetectionLoss(SimpleNamespace(model=[head], args=SimpleNamespace(**dict(hyp, distillation=True, distillation_loss="kl"))))
    # teacher lookup: neither source names both; a host map is refused (no host fallback); the channel count is checked
    prev = PL.set_teacher(None)
    try:
        with pytest.raises(y3d.Y3DError, match=r"teacher_emb.*set_teacher"):
            PL.teacher_map({"img": torch.zeros(1, 3, 8, 8)}, 16)
        with pytest.raises(y3d.Y3DError, match="HIP device"):
            PL.teacher_map({"teacher_emb": torch.zeros(1, 16, 2, 2)}, 16)
        PL.set_teacher(lambda img: (None, torch.zeros(img.shape[0], 16, 2, 2)))
        with pytest.raises(y3d.Y3DError, match="HIP device"):
            PL.teacher_map({"img": torch.zeros(1, 3, 8, 8)}, 16)
    finally:
        PL.set_teacher(prev)
