"""Mints the feature-distillation fixtures from the REFERENCE, run on the CPU with a stub teacher:

    python tools/make_golden_distill.py      # needs the reference checkout (oracle.ref_shim.import_reference)

tests/golden/distill.npz - `SupervisionLoss.forward_head` (utils/loss.py:1156-1188) itself.  The object is made with `object.__new__`
(its constructor loads the DINOv2 teacher over the network) and `foundation_model` is a function that returns a fixed random map.
Everything runs in float64 except the object centres (float32, as in training: the teacher pixel is computed in float32).  One
scenario per embedding width (128, 64), B = 4 images, anchors of three levels concatenated (4x10 + 2x5 + 1x4), a 6 x 16 teacher map
(non-square, the size of no level), image 256 x 128:
    image 0: 3 objects, mixed;   image 1: 1 object;   image 2: no object;   image 3: 4 objects whose centres sit exactly on .5
    teacher pixels (1.5 and 2.5: both round to 2) and outside the image (clamped)
Every image with objects has foreground anchors (the reference is 0 / 0 = NaN otherwise).  Cases: the three criteria, T of 1 and 2,
no_mixup on and off.  The `pix` arrays are the teacher pixels the reference itself used: a second run with the "mse" criterion, zero
embeddings and a teacher map whose channels 0 / 1 hold the x / y index returns them in its gradient.

tests/golden/loss3d_distill.npz - one whole `DetectLoss3d` call with `distillation: True` on the head maps and batch of
tests/golden/loss3d.npz, `SupervisionLoss.__init__` patched to install the stub: the 14 items, the gradients wrt the head maps and
the embeddings.  The fixtures hold data only.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
IMG_WH = (256, 128)
MAP_HW = (6, 16)
LEVELS = [(4, 10), (2, 5), (1, 4)]
CASES = [  # (name, width, criterion, T, no_mixup)
    ("soft_t2_nomix_c128", 128, "soft", 2.0, True), ("soft_t1_mix_c128", 128, "soft", 1.0, False),
    ("mse_t2_nomix_c128", 128, "mse", 2.0, True), ("cos_t2_mix_c128", 128, "cos", 2.0, False),
    ("soft_t2_mix_c64", 64, "soft", 2.0, False), ("mse_t1_mix_c64", 64, "mse", 1.0, False),
    ("cos_t1_nomix_c64", 64, "cos", 1.0, True), ("soft_t1_nomix_c64", 64, "soft", 1.0, True),
]
WEIGHT = 0.75


def scenario(C, seed):
    g = torch.Generator().manual_seed(seed)
    B, n, A = 4, 4, sum(h * w for h, w in LEVELS)
    W, H = IMG_WH
    gtc = torch.zeros(B, n, 2)
    gtc[0, :3] = torch.rand(3, 2, generator=g) * torch.tensor([W, H], dtype=torch.float32)
    gtc[1, :1] = torch.rand(1, 2, generator=g) * torch.tensor([W, H], dtype=torch.float32)
    # x / 256 * 16 and y / 128 * 6 are exact in float32 for these: 1.5 -> 2, 2.5 -> 2 (half to even); then the clamps on all four sides
    gtc[3] = torch.tensor([[24.0, 32.0], [40.0, 53.0], [-20.0, 140.0], [300.0, -3.0]])
    mask_gt = torch.tensor([[1, 1, 1, 0], [1, 0, 0, 0], [0, 0, 0, 0], [1, 1, 1, 1]]).bool()
    fg = torch.rand(B, A, generator=g) < 0.25
    fg[2] = False
    gi = torch.zeros(B, A, dtype=torch.long)
    for b in range(B):
        nv = int(mask_gt[b].sum())
        if nv:
            gi[b] = torch.randint(0, nv, (A,), generator=g)
            fg[b, b] = True  # at least one foreground anchor
            if b == 3:       # every object of image 3 is somebody's target
                fg[b, 10:14], gi[b, 10:14] = True, torch.arange(4)
    gi[~fg] = 0
    emb = torch.randn(B, C, A, generator=g, dtype=torch.float64)
    teach = torch.randn(B, C, *MAP_HW, generator=g, dtype=torch.float64)
    mixed = torch.tensor([1, 0, 0, 0]).bool()
    return dict(emb=emb, teacher=teach, gt_center=gtc, mask_gt=mask_gt, fg=fg, gt_idx=gi, mixed=mixed)


def supervisor(RL, teach, crit, T, no_mixup, B):
    S = object.__new__(RL.SupervisionLoss)
    S.T, S.weight, S.criterion, S.no_mixup = T, WEIGHT, crit, no_mixup
    S.loss = {"mse": torch.nn.MSELoss(), "cos": torch.nn.CosineEmbeddingLoss()}.get(crit)
    S.foundation_model = lambda imgs: (torch.zeros(B, 1, 1), teach)
    return S


def mint_forward_head(RL):
    out = {"img_wh": np.array(IMG_WH), "levels": np.array(LEVELS), "weight": np.array(WEIGHT)}
    imgs = torch.zeros(4, 3, IMG_WH[1], IMG_WH[0])
    for C, seed in ((128, 11), (64, 12)):
        sc = scenario(C, seed)
        for k, v in sc.items():
            out[f"in{C}/{k}"] = (v.float() if v.dtype == torch.float64 else v).numpy()  # float32 storage of the float64 inputs
        e32 = {k: (v.float().double() if v.dtype == torch.float64 else v) for k, v in sc.items()}
        # the teacher pixels the reference uses, read back from an "mse" gradient over a coordinate-coded map
        code = torch.zeros(4, C, *MAP_HW, dtype=torch.float64)
        code[:, 0] = torch.arange(MAP_HW[1], dtype=torch.float64).view(1, 1, -1)
        code[:, 1] = torch.arange(MAP_HW[0], dtype=torch.float64).view(1, -1, 1)
        z = torch.zeros_like(e32["emb"]).requires_grad_(True)
        S = supervisor(RL, code, "mse", 1.0, False, 4)
        S.forward_head(imgs, e32["gt_center"], z, e32["fg"], e32["gt_idx"], e32["mask_gt"], e32["mixed"]).backward()
        nfg = e32["fg"].sum(1).clamp(min=1).double().view(-1, 1, 1)
        pix = (-z.grad[:, :2] * nfg * C / (2 * WEIGHT)).round().long().permute(0, 2, 1)  # (B, A, 2) = (x, y)
        pix[~e32["fg"]] = -1
        out[f"in{C}/pix"] = pix.numpy()
        for name, Cc, crit, T, nomix in CASES:
            if Cc != C:
                continue
            emb = e32["emb"].clone().requires_grad_(True)
            S = supervisor(RL, e32["teacher"], crit, T, nomix, 4)
            l = S.forward_head(imgs, e32["gt_center"], emb, e32["fg"], e32["gt_idx"], e32["mask_gt"], e32["mixed"])
            assert torch.isfinite(l)
            l.backward()
            out[f"{name}/loss"], out[f"{name}/grad"] = l.detach().double().numpy(), emb.grad.numpy()
            out[f"{name}/cfg"] = np.array([C, ["soft", "mse", "cos"].index(crit), T, int(nomix)], np.float64)
            print(f"{name}: loss {float(l):.6f}, {int((emb.grad.abs().sum(1) > 0).sum())} rows")
    path = os.path.join(GOLDEN, "distill.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


def mint_whole_loss(RL):
    from ultralytics.nn.modules.head import v10Detect3d
    z = np.load(os.path.join(GOLDEN, "loss3d.npz"))
    strides = [float(s) for s in z["strides"]]
    batch = {k[6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("batch/")}
    o2m = [torch.from_numpy(z[f"o2m/{i}"]).requires_grad_(True) for i in range(3)]
    o2o = [torch.from_numpy(z[f"o2o/{i}"]).requires_grad_(True) for i in range(3)]
    B, C = o2m[0].shape[0], 16
    H, W = int(o2m[0].shape[2] * strides[0]), int(o2m[0].shape[3] * strides[0])
    g = torch.Generator().manual_seed(21)
    batch["img"] = torch.zeros(B, 3, H, W)
    teach = torch.randn(B, C, 5, 9, generator=g)
    e_m = [torch.randn(B, C, *t.shape[2:], generator=g).requires_grad_(True) for t in o2m]
    e_o = [torch.randn(B, C, *t.shape[2:], generator=g).requires_grad_(True) for t in o2o]
    chan = {k + "_c": 16 for k in ("cls", "o2d", "s2d", "o3d", "s3d", "hd", "dep", "dep_un")}
    hd = v10Detect3d(3, [16, 16, 16], False, chan, False, False, False, False, 3, False, False, 3, 3)
    hd.stride = torch.tensor(strides)

    class _M:
        pass

    m = _M()
    m.args, m.model, m.parameters = R.model_args(distillation=True), [hd], (lambda: iter([torch.zeros(1)]))

    def init(self, model):  # SupervisionLoss.__init__ without the DINOv2 download (loss.py:1139-1154)
        a = model.args
        self.T, self.weight, self.criterion, self.no_mixup = a.distillation_temp, a.distillation_weight, a.distillation_loss, a.distillation_no_mixup
        self.loss = None
        self.foundation_model = lambda imgs: (torch.zeros(B, 1, 1), teach)

    orig = RL.SupervisionLoss.__init__
    RL.SupervisionLoss.__init__ = init
    try:
        crit = RL.DetectLoss3d(m)
        with R.cpu_cuda_noop():
            loss, items = crit({"one2many": o2m, "one2one": o2o, "o2m_embs": e_m, "o2o_embs": e_o}, batch)
    finally:
        RL.SupervisionLoss.__init__ = orig
    assert torch.isfinite(items).all() and items.numel() == 14
    loss.backward()
    a = m.args
    out = {"teacher": teach.numpy(), "loss": loss.detach().numpy(), "items": items.detach().numpy(), "img_hw": np.array([H, W]),
           "hyp": np.array([a.distillation_temp, a.distillation_weight, ["soft", "mse", "cos"].index(a.distillation_loss), int(a.distillation_no_mixup)], np.float64)}
    for i in range(3):
        out[f"e_o2m/{i}"], out[f"e_o2o/{i}"] = e_m[i].detach().numpy(), e_o[i].detach().numpy()
        out[f"ge_o2m/{i}"], out[f"ge_o2o/{i}"] = e_m[i].grad.numpy(), e_o[i].grad.numpy()
        out[f"g_o2m/{i}"], out[f"g_o2o/{i}"] = o2m[i].grad.numpy(), o2o[i].grad.numpy()
    path = os.path.join(GOLDEN, "loss3d_distill.npz")
    np.savez_compressed(path, **out)
    print(f"items {items.tolist()}\nwrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    R.import_reference()
    from ultralytics.utils import loss as RL
    mint_forward_head(RL)
    mint_whole_loss(RL)
