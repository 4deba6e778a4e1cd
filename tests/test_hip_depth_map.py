"""GPU: foreground depth maps of the KITTI builders (csrc/kitti_depth_map.hip, the depth table of csrc/kitti_labels.hip,
kitti.augment_depth_maps / build_batch / DeviceSplit with `load_depth_maps`) against the restatements of tests/depth_map_ref.py -
Pillow's warp bit for bit - and the reference's own maps (tests/golden/kitti_depth_map.npz)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, has_gpu
from kitti_labels_tree import fixture, write_tree

import depth_map_ref as R
import yolov10_3d_amd as y3d
from yolov10_3d_amd import kitti

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]
DEV = "cuda"
KCASES = R.kernel_cases()
RUNS = ("mix", "nomix", "val")


def dev_mask(m):
    return torch.from_numpy(np.minimum(m, 255).astype(np.uint8)).to(DEV)


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", KCASES, ids=[c["name"] for c in KCASES])
def test_kernel_equals_the_restatement(case):
    out = kitti.augment_depth_maps([dev_mask(m) for m in case["masks"]], [None if q is None else dev_mask(q) for q in case["partners"]],
                                   case["flips"], list(case["trans_inv"]), torch.from_numpy(case["table"]).to(DEV), case["out_wh"],
                                   case["max_depth"], wide=case["wide"])
    W, H = case["out_wh"]
    assert out.dtype == torch.float32 and tuple(out.shape) == (3, H, W)
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), case["expect"].view(np.uint32)), f"{(got != case['expect']).sum()} pixels differ"


def test_kernel_writes_nothing_outside_its_output():
    """the output inside a larger sentinel-filled buffer, at an offset that leaves every row misaligned in turn"""
    c = KCASES[1]
    L, W, H, B = y3d.lib(), c["out_wh"][0], c["out_wh"][1], 3
    masks = [dev_mask(m) for m in c["masks"]]
    parts = [None if q is None else dev_mask(q) for q in c["partners"]]
    i64 = lambda v: torch.tensor(v, dtype=torch.int64).to(DEV)
    mask, mask2 = i64([t.data_ptr() for t in masks]), i64([0 if q is None else q.data_ptr() for q in parts])
    hw = torch.tensor([list(t.shape) for t in masks], dtype=torch.int32).to(DEV)
    fl = torch.tensor([int(f) for f in c["flips"]], dtype=torch.int32).to(DEV)
    ti = torch.from_numpy(c["trans_inv"]).to(DEV)
    wd = torch.tensor([[int(a), int(b)] for a, b in c["wide"]], dtype=torch.uint8).to(DEV)
    tab = torch.from_numpy(c["table"]).to(DEV)
    xy = torch.empty(B, W + H, dtype=torch.int32, device=DEV)
    for lead in (5, 8):  # floats ahead of the output: off and on a 16-byte boundary
        buf = torch.full((lead + B * H * W + 11,), -7.0, dtype=torch.float32, device=DEV)
        L.kitti_depth_map(mask.data_ptr(), mask2.data_ptr(), None, None, None, 0, wd.data_ptr(), hw.data_ptr(), fl.data_ptr(), ti.data_ptr(),
                          tab.data_ptr(), B, H, W, 90, c["max_depth"], xy.data_ptr(), buf.data_ptr() + 4 * lead, y3d.ops.stream())
        got = buf.cpu().numpy()
        assert (got[:lead] == -7.0).all() and (got[lead + B * H * W:] == -7.0).all()
        assert np.array_equal(got[lead:lead + B * H * W].reshape(B, H, W), c["expect"])


def test_kernel_refuses_bad_arguments():
    L = y3d.lib()
    one = torch.zeros(16, dtype=torch.int64, device=DEV)
    args = lambda B, H, W, side: (one.data_ptr(), None, None, None, None, 0, None, one.data_ptr(), one.data_ptr(), one.data_ptr(), one.data_ptr(),
                                  B, H, W, side, 120.0, one.data_ptr(), one.data_ptr(), y3d.ops.stream())
    for bad, word in (((0, 8, 8, 8), "B ="), ((1, 0, 8, 8), "resolution"), ((1, 8, 0, 8), "resolution"), ((1, 8, 8, 32768), "32768"),
                      ((1, 32768, 8, 8), "32768")):
        with pytest.raises(y3d.Y3DError, match=word):
            L.kitti_depth_map(*args(*bad))
    m = torch.zeros(8, 8, dtype=torch.uint8)
    with pytest.raises(y3d.Y3DError, match="HIP device"):  # a host mask
        kitti.augment_depth_maps([m], [None], [False], [np.eye(2, 3)], torch.zeros(1, 2, 64, device=DEV), (8, 8))
    with pytest.raises(y3d.Y3DError, match="line_depth"):
        kitti.augment_depth_maps([m.to(DEV)], [None], [False], [np.eye(2, 3)], torch.zeros(1, 2, 64), (8, 8))


# ---- the rebuilt tree --------------------------------------------------------------------------------------------------------------
def write_masks(root, z, sub="training/image_2"):
    from PIL import Image
    os.makedirs(os.path.join(root, sub), exist_ok=True)
    for i in range(len(z["label_text"])):
        W, H = (int(v) for v in z["frame_wh"][i])
        m = R.synthetic_mask(R.parse_label(str(z["label_text"][i])), i, W, H, R.mask_bits(i))
        Image.fromarray(m).save(os.path.join(root, sub, f"{i:06d}_seg.png"))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    z = fixture()
    root = write_tree(str(tmp_path_factory.mktemp("kitti_depth")), z, images=True)
    write_masks(root, z)
    return root, z, np.load(os.path.join(GOLDEN, "kitti_depth_map.npz"))


@pytest.fixture(scope="module")
def restated(tree):
    root, z, zd = tree
    return {name: R.builder_maps(z, zd, name) for name in RUNS}


def run_args(zd, name, **over):
    return str(zd[f"{name}/mode"]), kitti.data_args(mixup=float(zd[f"{name}/mixup"]), **over), int(zd[f"{name}/seed"]), [int(i) for i in zd[f"{name}/items"]]


@pytest.mark.parametrize("name", RUNS)
def test_depth_table_and_label_rows(tree, restated, name):
    """the (B, 2, 64) table of the launch equals the restatement bit for bit; its label rows are y3d_kitti_encode_labels' rows"""
    root, z, zd = tree
    mode, args, seed, items = run_args(zd, name)
    lab = lambda i: kitti.read_label(os.path.join(root, "training/label_2", f"{i:06d}.txt"))
    P2 = lambda i: kitti.read_calib(os.path.join(root, "training/calib", f"{i:06d}.txt"))
    flips = [bool(f) for f in zd[f"{name}/flip"]]
    packed = kitti.pack_labels([lab(i) for i in items], [lab(int(p)) if p >= 0 else None for p in zd[f"{name}/partner"]],
                               [z["flip_P2"][i] if f else P2(i) for i, f in zip(items, flips)], list(zd[f"{name}/trans"]), flips,
                               list(zd[f"{name}/scale"]), [z["frame_wh"][i] for i in items], DEV)
    plain = kitti.encode_labels(packed, kitti.RESOLUTION, 1.0, 120.0, False)
    both = kitti.encode_labels(packed, kitti.RESOLUTION, 1.0, 120.0, False, depths=True)
    assert "line_depth" not in plain and set(both) == set(plain) | {"line_depth"}
    for k in plain:
        assert torch.equal(plain[k], both[k]), k
    got = both["line_depth"].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), restated[name][2].view(np.uint32))
    cam = kitti.encode_labels(packed, kitti.RESOLUTION, 1.0, 120.0, True, depths=True)  # never the camera distance
    assert torch.equal(cam["line_depth"], both["line_depth"])


@pytest.mark.parametrize("name", RUNS)
def test_builders_equal_each_other_and_the_reference(tree, restated, name):
    root, z, zd = tree
    mode, args, seed, items = run_args(zd, name, load_depth_maps=True)
    np.random.seed(seed)
    a = kitti.build_batch(root, items, args, DEV, mode=mode)
    split = kitti.DeviceSplit(root, mode, DEV, load_depth_maps=True, workers=4)
    assert all(int(o) % 16 == 0 for o in split.mask_offsets)
    np.random.seed(seed)
    b = kitti.build_batch(split, items, args, DEV, mode=mode)
    for batch in (a, b):
        dm = batch["depth_map"]
        assert dm.dtype == torch.float32 and tuple(dm.shape) == (len(items), 384, 1280) and dm.device.type == "cuda"
    assert torch.equal(a["depth_map"], b["depth_map"])
    got = a["depth_map"].cpu().numpy()
    want = zd[f"{name}/depth_map"].astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{(got != want).sum()} pixels differ from the reference"
    assert np.array_equal(got, restated[name][1])
    for k in ("img", "cls", "bboxes", "depth", "counts", "calib", "mixed"):
        assert torch.equal(a[k], b[k]), k


def test_switch_off_changes_nothing(tree):
    root, z, zd = tree
    mode, args, seed, items = run_args(zd, "mix")
    assert args.load_depth_maps is False
    split = kitti.DeviceSplit(root, mode, DEV, load_depth_maps=True, workers=4)
    plain = kitti.DeviceSplit(root, mode, DEV, workers=4)
    assert not hasattr(plain, "mask_arena")
    batches = []
    for src, kw in ((root, {}), (split, {}), (plain, {}), (root, dict(load_depth_maps=True))):
        np.random.seed(seed)
        batches.append(kitti.build_batch(src, items, kitti.data_args(mixup=args.mixup, **kw), DEV, mode=mode))
    off, on = batches[0], batches[3]
    assert all("depth_map" not in b for b in batches[:3]) and set(on) == set(off) | {"depth_map"}
    for other in batches[1:]:
        for k, v in off.items():
            if torch.is_tensor(v):
                assert torch.equal(v, other[k]), k
            elif k != "info":
                assert all(np.array_equal(x, y) for x, y in zip(v, other[k])), k


def test_refusals(tree, tmp_path):
    root, z, zd = tree
    import shutil
    from PIL import Image
    mode, args, seed, items = run_args(zd, "val", load_depth_maps=True)
    with pytest.raises(y3d.Y3DError, match="load_depth_maps=True"):  # a resident split built without masks
        kitti.build_batch(kitti.DeviceSplit(root, mode, DEV, workers=4), items, args, DEV, mode=mode)
    with pytest.raises(y3d.Y3DError, match="HIP device"):
        kitti.build_batch(root, items, args, "cpu", mode=mode)
    bad = str(tmp_path / "bad")
    shutil.copytree(root, bad)
    seg = lambda i: os.path.join(bad, "training/image_2", f"{i:06d}_seg.png")
    os.remove(seg(items[1]))
    with pytest.raises(y3d.Y3DError, match=f"{items[1]:06d}"):  # a missing mask names its frame
        kitti.build_batch(bad, items, args, DEV, mode=mode)
    with pytest.raises(y3d.Y3DError, match=f"{items[1]:06d}"):
        kitti.DeviceSplit(bad, mode, DEV, load_depth_maps=True, workers=4)
    W, H = (int(v) for v in z["frame_wh"][items[1]])
    Image.fromarray(np.zeros((H - 1, W), np.uint8)).save(seg(items[1]))
    with pytest.raises(y3d.Y3DError, match=f"mask of frame {items[1]:06d}"):  # a mask of another size
        kitti.build_batch(bad, items, args, DEV, mode=mode)
    Image.fromarray(np.zeros((H, W, 3), np.uint8)).save(seg(items[1]))
    with pytest.raises(y3d.Y3DError, match="single channel"):  # a three-channel mask
        kitti.build_batch(bad, items, args, DEV, mode=mode)
    # the masks of a deepseg directory win over the ones next to the images
    write_masks(bad, z, "deepseg/training/image_2")
    assert kitti.seg_path(os.path.join(bad, "training"), 3).endswith("deepseg/training/image_2/000003_seg.png")
    np.random.seed(seed)
    ok = kitti.build_batch(bad, items, args, DEV, mode=mode)
    assert np.array_equal(ok["depth_map"].cpu().numpy(), zd["val/depth_map"].astype(np.float32))
    # both arenas share the byte budget, checked before anything is decoded
    with pytest.raises(y3d.Y3DError, match="masks need"):
        kitti.DeviceSplit(root, mode, DEV, load_depth_maps=True, max_bytes=kitti.DeviceSplit(root, mode, DEV, workers=4).nbytes + 1000)
