"""Times what `load_depth_maps` adds to a KITTI batch, and the foreground depth map loss (profiles/depth_map_bench.txt).

    python tools/depth_map_bench.py [--batch 32] [--reps 200] [--host-only] [--package-root DIR]

A resident split over the synthetic tree of tests/golden/kitti_labels.npz (12 frames at KITTI sizes, masks of
tests/depth_map_ref.synthetic_mask) builds batches of `--batch` positions at 1280 x 384.  Device times are event-timed over `--reps`
launches after a warm-up: the label encoder with and without the depth table, the depth map launch pair (index + map), and
ForegroundDepthMapLoss forward + backward at (batch, 81, 24, 80).  Host time: `DeviceSplit.build_batch` with the switch off and on
(wall clock per call, the stream drained only at the end of the window).  --host-only measures just the switch-off host time, and
--package-root imports the package from another checkout, so two versions can be run alternately on one machine.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COPY_TBPS = 6.29  # the copy rate DESIGN quotes for this chip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--package-root", default=ROOT)
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import yolov10_3d_amd as y3d  # before the test helpers: their conftest puts this repository's root first on sys.path
    from yolov10_3d_amd import kitti
    import depth_map_ref as R
    from kitti_labels_tree import fixture, write_tree
    assert os.path.abspath(kitti.__file__).startswith(os.path.abspath(a.package_root)), kitti.__file__
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = "cuda"
    z = fixture()
    root = write_tree(tempfile.mkdtemp(prefix="y3d_depth_bench_"), z, images=True)
    n = len(z["label_text"])
    if not a.host_only:
        from PIL import Image
        for i in range(n):
            W, H = (int(v) for v in z["frame_wh"][i])
            m = R.synthetic_mask(R.parse_label(str(z["label_text"][i])), i, W, H, R.mask_bits(i))
            Image.fromarray(m).save(os.path.join(root, "training/image_2", f"{i:06d}_seg.png"))
    B, reps = a.batch, a.reps
    items = [i % n for i in range(B)]
    off = kitti.data_args()

    def host_time(split, args, label):
        np.random.seed(0)
        for _ in range(10):
            split.build_batch(items, args)
        torch.cuda.synchronize()
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(reps // 5):
                split.build_batch(items, args)
            t.append((time.perf_counter() - t0) / (reps // 5) * 1e3)
            torch.cuda.synchronize()
        print(f"host  build_batch {label}: {np.median(t):.3f} ms per call (5 windows: min {min(t):.3f}, max {max(t):.3f})")

    if a.host_only:
        host_time(kitti.DeviceSplit(root, "train", dev), off, f"switch off [{a.package_root}]")
        return
    split = kitti.DeviceSplit(root, "train", dev, load_depth_maps=True)
    on = kitti.data_args(load_depth_maps=True)

    def dev_time(fn, label, nbytes=None):
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / reps * 1e3
        rate = "" if nbytes is None else f", {nbytes / us / 1e6:.3f} TB/s = {nbytes / us / 1e6 / COPY_TBPS * 100:.1f} % of the {COPY_TBPS} TB/s copy rate"
        print(f"device {label}: {us:.1f} us per call{rate}")
        return us

    np.random.seed(0)
    draws = kitti.sample_augment(len(split), items, split.frame_info, on, "train")
    host, d = split._ring.upload(kitti.draw_table(items, draws))
    plan = kitti.plan_batch(split, host, d)
    packed = dict(rec=split.rec, img_i=plan["img_i"], img_f=plan["img_f"], mean_size=split.mean_size)
    t0 = dev_time(lambda: kitti.encode_labels(packed), "label encoder")
    t1 = dev_time(lambda: kitti.encode_labels(packed, depths=True), "label encoder + depth table")
    lab = kitti.encode_labels(packed, depths=True)
    W, H = kitti.RESOLUTION
    mask_bytes = sum(int(split._hw[p].prod()) * (2 if dd["mixed"] else 1) for p, dd in zip(items, draws))
    traffic = B * H * W * 4 + mask_bytes
    dev_time(lambda: kitti._depth_map_launch(B, kitti.RESOLUTION, 120.0, int(split._hw.max()), split.device, arena=split.mask_arena,
                                             mask_off=split.mask_off, wide=split.mask_wide, draws=d, draw_w=16, hw=plan["hw"],
                                             flip=plan["flip"], trans_inv=plan["trans_inv"], line_depth=lab["line_depth"]),
             f"depth map launches (B = {B}, {B * H * W * 4 / 1e6:.1f} MB written, {mask_bytes / 1e6:.1f} MB of masks read, output allocation included)",
             traffic)
    print(f"device depth table adds {t1 - t0:+.1f} us to the label encoder")
    from yolov10_3d_amd import loss as PL
    crit = PL.ForegroundDepthMapLoss(on)
    for dt in (torch.float32, torch.bfloat16):
        for cl in (False, True):
            zl = torch.randn(B, 81, H // 16, W // 16, device=dev, dtype=dt)
            zl = (zl.contiguous(memory_format=torch.channels_last) if cl else zl).requires_grad_(True)
            dm = kitti.build_batch(split, items, on, dev)["depth_map"]

            def step():
                zl.grad = None
                crit(zl, dm).backward()

            dev_time(step, f"fgdm loss forward + backward {tuple(zl.shape)} {dt} {'channels_last' if cl else 'contiguous'}")
    host_time(split, off, "switch off")
    host_time(split, on, "switch on ")


if __name__ == "__main__":
    main()
