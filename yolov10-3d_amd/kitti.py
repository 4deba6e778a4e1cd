"""KITTI decode of the post-processed detections on the device — the eval tail behind `v10_3Dpostprocess`.

Mirrors `KITTIDataset.decode_preds` / `decode_preds_eval` (data/datasets/kitti.py:515-576), which the reference's validator calls
from `_prepare_preds` (models/yolov10_3D/val.py:210-214) on CPU with a python loop and `.item()` per detection: heading-bin argmax +
residual -> alpha, size residual + class mean size, centre back-projection through the (inverse-affine'd) calibration, rotation_y,
score = sigmoid(cls) * exp(-depth log-variance), threshold.  Here it is one launch over all B*K rows (`y3d_kitti_decode`).

Further down: the labels of a built batch back to 3D boxes (`decode_batch_device`, `decode_batch`: the reference's `decode_batch`,
one launch of `y3d_decode_labels`), the one-to-many depth fusion, the image and label sides of the training / validation batches (`build_batch`), the same
batches from a split decoded once and kept on the device (`DeviceSplit`, `plan_batch`, `epoch_indices`), the unlabelled test split
(`build_test_batch`, which `predict.Predictor3d.predict_split` reads) and `save_results`, the writer of the files a KITTI submission
and `kitti_eval.eval_from_scratch` read.
"""
from __future__ import annotations

import torch

from . import ops
from ._lib import Y3DError, lib
from .resident import ALIGN, DrawRing, ResidentSplit, check_plan, epoch_indices, fill_arena, span_table, upload  # noqa: F401  (re-exported)

# (h, w, l) per class, kitti.py:38-41
CLS_MEAN_SIZE = ((1.52563191462, 1.62856739989, 3.88311640418), (1.76255119, 0.66068622, 0.84422524), (1.73698127, 0.59706367, 1.76282397))


def _calib_rows(calibs, B, dev):
    if torch.is_tensor(calibs):
        c = calibs.to(dev, torch.float64).reshape(B, 6)
    else:  # the reference's Calibration objects (kitti_utils.py:178-196) or anything with the same six attributes
        c = torch.tensor([[float(k.cu), float(k.cv), float(k.fu), float(k.fv), float(k.tx), float(k.ty)] for k in calibs], dtype=torch.float64, device=dev)
    if c.shape != (B, 6):
        raise Y3DError(f"decode_preds: {B} images but calibration rows of shape {tuple(c.shape)}")
    return c.contiguous()


def decode_preds_device(preds, calibs, ratio_pad, inv_trans, undo_augment=True, threshold=0.001, cls_mean_size=CLS_MEAN_SIZE,
                        use_camera_dis=False):
    """preds (B, K, 37) on the device -> rows (B, K, 14) float64 [cls, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, score] and
    keep (B, K) bool, both on the device, no host synchronisation.  ratio_pad: (B, 2, 2) as collated (kitti.py:404, 431) or (B, 2)."""
    if preds.dim() != 3 or preds.shape[-1] != 37:
        raise Y3DError(f"decode_preds: expected (B, K, 37) predictions, got {tuple(preds.shape)}")
    dev = preds.device
    if dev.type != "cuda":
        raise Y3DError("decode_preds needs the predictions on a HIP device")
    B, K, _ = preds.shape
    p = preds.detach().float().contiguous()
    calib = _calib_rows(calibs, B, dev)
    rp = torch.as_tensor(ratio_pad).to(dev, torch.float64)
    ratio = (rp[:, 0] if rp.dim() == 3 else rp).reshape(B, 2).contiguous()
    inv = None
    if undo_augment:
        inv = torch.stack([torch.as_tensor(t, dtype=torch.float64).reshape(2, 3) for t in inv_trans]).to(dev).contiguous()
        if inv.shape[0] != B:
            raise Y3DError(f"decode_preds: {B} images but {inv.shape[0]} inverse transforms")
    ms = torch.as_tensor(cls_mean_size, dtype=torch.float64).reshape(-1, 3).to(dev).contiguous()
    out = torch.empty(B, K, 14, dtype=torch.float64, device=dev)
    keep = torch.empty(B, K, dtype=torch.uint8, device=dev)
    lib().kitti_decode(p.data_ptr(), B, K, calib.data_ptr(), ratio.data_ptr(), inv.data_ptr() if inv is not None else None, ms.data_ptr(),
                       ms.shape[0], int(bool(use_camera_dis)), float(threshold), out.data_ptr(), keep.data_ptr(), ops.stream())
    return out, keep.bool()


def decode_preds(preds, calibs, im_files, ratio_pad, inv_trans, undo_augment=True, threshold=0.001, cls_mean_size=CLS_MEAN_SIZE,
                 use_camera_dis=False):
    """kitti.py:519-576: {im_file: [[cls, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, score], ...]} (one device->host copy)"""
    rows, keep = decode_preds_device(preds, calibs, ratio_pad, inv_trans, undo_augment, threshold, cls_mean_size, use_camera_dis)
    rows, keep = rows.cpu(), keep.cpu()
    return {f: rows[i][keep[i]].tolist() for i, f in enumerate(im_files)}


def decode_preds_eval(preds, calibs, im_files, ratio_pad, inv_trans, undo_augment=True, threshold=0.001, **kw):
    """kitti.py:515-517"""
    return decode_preds(preds, calibs, im_files, ratio_pad, inv_trans, undo_augment=undo_augment, threshold=threshold, **kw)


# ------------------------------------------------------------------------------------------------------------------------------
# the labels of a batch back to 3D boxes: KITTIDataset.decode_batch (data/datasets/kitti.py:469-513) on the device
# ------------------------------------------------------------------------------------------------------------------------------
_LABEL_KEYS = ("cls", "bboxes", "center_3d", "size_3d", "depth", "heading_bin", "heading_res", "batch_idx")  # y3d_decode_labels' order
_LABEL_DTYPES = {"cls": torch.int64, "bboxes": torch.float64, "center_3d": torch.float64, "size_3d": torch.float64, "depth": torch.float64,
                 "heading_bin": torch.int64, "heading_res": torch.float64, "batch_idx": torch.float32}
_LABEL_WIDTH = {"cls": 1, "bboxes": 4, "center_3d": 2, "size_3d": 3, "depth": 1, "heading_bin": 1, "heading_res": 1, "batch_idx": 1}


def _calib6(calibs, B, dev, what):
    """(B, 6) float64 on the device from a tensor, a list of six-tuples (`calib_params`) or the reference's Calibration objects"""
    import numpy as np
    if torch.is_tensor(calibs):
        if not calibs.is_cuda:
            raise Y3DError(f"{what}: a calibration tensor must live on a HIP device (or pass a list of six-tuples)")
        c = calibs.to(torch.float64)
    else:
        six = [[float(getattr(k, a)) for a in ("cu", "cv", "fu", "fv", "tx", "ty")] if hasattr(k, "cu") else [float(v) for v in k] for k in calibs]
        if any(len(r) != 6 for r in six):
            raise Y3DError(f"{what}: a calibration is (cu, cv, fu, fv, tx, ty)")
        c = upload(np.array(six, np.float64).reshape(-1, 6), dev, torch.float64)
    if c.numel() != B * 6:
        raise Y3DError(f"{what}: {B} images but calibration rows of shape {tuple(c.shape)}")
    return c.reshape(B, 6).contiguous()


def p2_device(P2, B, dev):
    """(B, 3, 4) float64 on the device from a device tensor (any float dtype), an array or a list of 3 x 4 matrices"""
    import numpy as np
    if torch.is_tensor(P2):
        if not P2.is_cuda:
            raise Y3DError("decode_batch: a P2 tensor must live on a HIP device (or pass arrays)")
        P = P2.to(torch.float64)
    else:
        P = upload(np.stack([np.asarray(p, np.float64).reshape(3, 4) for p in P2]), dev, torch.float64)
    if P.numel() != B * 12:
        raise Y3DError(f"decode_batch: {B} images but P2 of shape {tuple(P.shape)} (one 3 x 4 matrix each)")
    return P.reshape(B, 3, 4).contiguous()


def decode_labels(labels, counts_in, ori_shape, calib, ratio_pad, trans_inv, P2, mean_size, undo_augment=True, use_camera_dis=False,
                  R=None, out=None):
    """`y3d_decode_labels` on device tensors alone: no upload, no allocation beyond the outputs (none with `out`), no wait for the
    device, so the call can be captured into a graph.  labels: the per-box tensors `cls`, `bboxes`, `center_3d`, `size_3d`, `depth`,
    `heading_bin`, `heading_res`, `batch_idx` in encode_labels' dtypes.  counts_in (B,) int32: the static layout (`max_objs` =
    rows / B per image); None: the ragged one (image b owns the rows with batch_idx == b).  ori_shape (B, 2) float64 (height, width),
    calib (B, 6), ratio_pad (B, 2, 2) or (B, 2), trans_inv (B, 2, 3) or None, P2 (B, 3, 4) float64 or None, mean_size (nc, 3), all
    float64.  out: optionally (rows (B, R, 14), corners3d (B, R, 8, 3), corners_img (B, R, 8, 2) or None, counts (B,) int32).
    -> (rows, corners3d, corners_img or None, counts)"""
    B = int(ori_shape.shape[0]) if torch.is_tensor(ori_shape) and ori_shape.dim() == 2 else 0
    if B < 1 or tuple(ori_shape.shape) != (B, 2):
        raise Y3DError("decode_labels: ori_shape must be a (B, 2) tensor of (height, width), B >= 1")
    dev = ori_shape.device
    missing = [k for k in _LABEL_KEYS if k not in labels]
    if missing:
        raise Y3DError(f"decode_labels: the batch lacks its per-box keys {missing}")
    per_image = {"ori_shape": ori_shape, "calib": calib, "ratio_pad": ratio_pad, "mean_size": mean_size}
    if trans_inv is not None:
        per_image["trans_inv"] = trans_inv
    if P2 is not None:
        per_image["P2"] = P2
    for k, t in per_image.items():
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
            raise Y3DError(f"decode_labels: {k} must be a contiguous float64 tensor on a HIP device (no host fallback)")
    N = int(labels["cls"].shape[0]) if torch.is_tensor(labels["cls"]) else -1
    for k in _LABEL_KEYS:
        t = labels[k]
        if not torch.is_tensor(t) or not t.is_cuda:
            raise Y3DError(f"decode_labels: {k} must be a tensor on a HIP device (no host fallback)")
        if t.dtype != _LABEL_DTYPES[k] or not t.is_contiguous():
            raise Y3DError(f"decode_labels: {k} must be a contiguous {str(_LABEL_DTYPES[k]).replace('torch.', '')} tensor, got {t.dtype}")
        if t.numel() != N * _LABEL_WIDTH[k]:
            raise Y3DError(f"decode_labels: {k} of shape {tuple(t.shape)} next to {N} rows of cls")
    if calib.numel() != B * 6 or ratio_pad.numel() not in (B * 2, B * 4) or mean_size.dim() != 2 or mean_size.shape[1] != 3 or not mean_size.shape[0]:
        raise Y3DError(f"decode_labels: {B} images but calib {tuple(calib.shape)}, ratio_pad {tuple(ratio_pad.shape)}, mean_size {tuple(mean_size.shape)}")
    if (trans_inv is not None and trans_inv.numel() != B * 6) or (P2 is not None and P2.numel() != B * 12):
        raise Y3DError(f"decode_labels: {B} images need trans_inv (B, 2, 3) and P2 (B, 3, 4)")
    if undo_augment and trans_inv is None:
        raise Y3DError("decode_labels: undo_augment needs trans_inv")
    max_objs = 0
    if counts_in is not None:
        if not torch.is_tensor(counts_in) or not counts_in.is_cuda or counts_in.dtype != torch.int32 or tuple(counts_in.shape) != (B,):
            raise Y3DError(f"decode_labels: counts must be a (B,) int32 tensor on a HIP device, B = {B}")
        if N < B or N % B:
            raise Y3DError(f"decode_labels: a static layout of {N} rows does not divide into {B} images")
        max_objs = N // B
    R = MAX_OBJS if R is None else int(R)
    if R < 1:
        raise Y3DError(f"decode_labels: R = {R} slots per image")
    if out is None:
        e = lambda *s, dt=torch.float64: torch.empty(*s, dtype=dt, device=dev)
        out = (e(B, R, 14), e(B, R, 8, 3), e(B, R, 8, 2) if P2 is not None else None, e(B, dt=torch.int32))
    rows, c3, ci, counts = out
    if tuple(rows.shape) != (B, R, 14) or tuple(c3.shape) != (B, R, 8, 3) or tuple(counts.shape) != (B,) or (ci is not None and tuple(ci.shape) != (B, R, 8, 2)):
        raise Y3DError(f"decode_labels: outputs must be (B, R, 14), (B, R, 8, 3), (B, R, 8, 2), (B,) with B = {B}, R = {R}")
    if (ci is None) != (P2 is None):
        raise Y3DError("decode_labels: corners_img goes with P2 (both or neither)")
    for t, dt in ((rows, torch.float64), (c3, torch.float64), (ci, torch.float64), (counts, torch.int32)):
        if t is not None and (not t.is_cuda or t.dtype != dt or not t.is_contiguous()):
            raise Y3DError("decode_labels: the outputs must be contiguous float64 (counts: int32) tensors on a HIP device")
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    lib().decode_labels(*[ptr(labels[k]) for k in _LABEL_KEYS], ptr(counts_in), N, max_objs, B, ori_shape.data_ptr(), calib.data_ptr(),
                        ratio_pad.data_ptr(), 4 if ratio_pad.numel() == B * 4 else 2, ptr(trans_inv), ptr(P2), mean_size.data_ptr(),
                        int(mean_size.shape[0]), int(bool(use_camera_dis)), int(bool(undo_augment)), R, rows.data_ptr(), c3.data_ptr(), ptr(ci),
                        counts.data_ptr(), ops.stream())
    return rows, c3, ci, counts


def batch_labels(batch):
    """the per-box tensors of a built batch in y3d_decode_labels' dtypes (the ragged form holds collate_fn's promoted dtypes, widened here
    exactly) and its `counts` (static layout) or None (ragged)"""
    missing = [k for k in _LABEL_KEYS if k not in batch]
    if missing:
        raise Y3DError(f"decode_batch: the batch lacks its per-box keys {missing}")
    labels = {}
    for k in _LABEL_KEYS:
        t = batch[k]
        if not torch.is_tensor(t) or not t.is_cuda:
            raise Y3DError(f"decode_batch: batch[{k!r}] must be a tensor on a HIP device (no host fallback)")
        labels[k] = t.to(_LABEL_DTYPES[k]).contiguous()
    return labels, batch.get("counts")


def decode_batch_device(batch, calibs, P2=None, undo_augment=True, cls_mean_size=CLS_MEAN_SIZE, use_camera_dis=False, max_objs=None):
    """`KITTIDataset.decode_batch` (kitti.py:469-513) for a batch of `build_batch` (either layout) on the device, one launch
    (`y3d_decode_labels`) and no read-back.  calibs: the ORIGINAL images' (cu, cv, fu, fv, tx, ty) as (B, 6) device tensor or a list of
    six-tuples (`calib_params`; uploaded once); `trans_inv` is taken from `batch["info"]`; P2: the original images' (B, 3, 4)
    projections (device tensor, array or list), or None.  -> rows (B, R, 14) float64 [cls, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry,
    1], corners3d (B, R, 8, 3), corners_img (B, R, 8, 2) in original-image pixels (None without P2), counts (B,) int32; image b's
    boxes are its first counts[b] slots in label order, the rest zeros.  R = the static layout's rows per image, or
    min(rows of the batch, max_objs) for the ragged one (max_objs None: MAX_OBJS).  A class outside the mean-size table stays in
    column 0 (`decode_batch` raises on it); a box behind the camera is decoded like any other (its projected corners are the plain
    quotient; `plot.box3d_segments` clips at the near plane)."""
    import numpy as np
    if "ori_shape" not in batch or "ratio_pad" not in batch or "info" not in batch:
        raise Y3DError("decode_batch: the batch lacks ori_shape, ratio_pad or info")
    labels, counts_in = batch_labels(batch)
    dev = labels["cls"].device
    B = len(batch["ori_shape"])
    if B < 1 or len(batch["info"]) != B:
        raise Y3DError(f"decode_batch: {B} ori_shape entries, {len(batch['info'])} info entries")
    ori = upload(np.array([[float(s[0]), float(s[1])] for s in batch["ori_shape"]], np.float64).reshape(B, 2), dev, torch.float64)
    calib = _calib6(calibs, B, dev, "decode_batch")
    rp = batch["ratio_pad"]
    if not torch.is_tensor(rp) or not rp.is_cuda:
        raise Y3DError("decode_batch: batch['ratio_pad'] must be a tensor on a HIP device (no host fallback)")
    rp = rp.to(torch.float64).contiguous()
    inv = None
    if undo_augment:
        inv = upload(np.stack([np.asarray(i["trans_inv"], np.float64).reshape(2, 3) for i in batch["info"]]), dev, torch.float64)
    if P2 is not None:
        P2 = p2_device(P2, B, dev)
    ms = cls_mean_size if torch.is_tensor(cls_mean_size) else upload(np.asarray(cls_mean_size, np.float64).reshape(-1, 3), dev, torch.float64)
    ms = ms.to(dev, torch.float64).reshape(-1, 3).contiguous()
    N = int(labels["cls"].shape[0])
    if counts_in is not None:
        if N < B or N % B:
            raise Y3DError(f"decode_batch: a static layout of {N} rows does not divide into {B} images")
        R = N // B
    else:
        R = max(1, min(N, MAX_OBJS if max_objs is None else int(max_objs)))
    return decode_labels(labels, counts_in, ori, calib, rp, inv, P2, ms, undo_augment, use_camera_dis, R)


def decode_batch(batch, calibs, undo_augment=True, cls_mean_size=CLS_MEAN_SIZE, use_camera_dis=False, max_objs=None):
    """kitti.py:469-513: {im_file: [[cls, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, 1], ...]} after one read-back.  A label whose class
    lies outside the mean-size table raises (the reference's IndexError)."""
    rows, _, _, counts = decode_batch_device(batch, calibs, None, undo_augment, cls_mean_size, use_camera_dis, max_objs)
    host = torch.cat((rows.reshape(rows.shape[0], -1), counts.to(rows.dtype).unsqueeze(1)), 1).cpu()
    nc = len(cls_mean_size)
    out = {}
    for i, f in enumerate(batch["im_file"]):
        n = int(host[i, -1])
        r = host[i, :n * 14].reshape(n, 14).tolist()
        for row in r:
            if not 0 <= row[0] < nc:
                raise Y3DError(f"decode_batch: {f} holds class {row[0]:g}, outside the mean-size table of {nc} classes")
            row[0], row[13] = int(row[0]), 1
        out[f] = r
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# f2: one-to-many depth fusion of the validator (models/yolov10_3D/val.py:78-102)
# ------------------------------------------------------------------------------------------------------------------------------
def aggregate_o2m_preds(predsO, predsM, thres=0.1, iou_thres=0.9, nprop=500):
    """`YOLOv10_3DDetectionValidator.aggregate_o2m_preds`: predsO (B, K, 37) / predsM (B, KM, 37) post-processed rows (regression |
    score | label, val.py:47-54) on the device -> predsO with every depth replaced by the mode of the weighted kernel density of the
    matching one-to-many depths.  One HIP launch (`y3d_kde_depth_fusion`, one block per detection); the reference loops over the
    detections in Python and fits a scikit-learn KernelDensity per detection on the host."""
    if predsO.dim() != 3 or predsM.dim() != 3 or predsO.shape[0] != predsM.shape[0] or predsO.shape[2] != predsM.shape[2]:
        raise Y3DError(f"aggregate_o2m_preds: expected (B, K, C) and (B, KM, C), got {tuple(predsO.shape)} / {tuple(predsM.shape)}")
    if predsO.device.type != "cuda":
        raise Y3DError("aggregate_o2m_preds needs the predictions on a HIP device")
    O, M = predsO.detach().float().contiguous(), predsM.detach().float().contiguous()
    out = torch.empty_like(O)
    B, K, C = O.shape
    lib().kde_depth_fusion(O.data_ptr(), B, K, M.data_ptr(), M.shape[1], C, float(thres), float(iou_thres), int(nprop), out.data_ptr(), ops.stream())
    return out


def depth_from_map(rows, depth_maps):
    """`YOLOv10_3DDetectionValidator.dino_depth_pred` (val.py:61-76) without the depth network: rows (B, K, C) post-processed rows and
    depth_maps (B, Hm, Wm) on the device -> a new (B, K, C) float32 tensor, rows with the depth column (C - 4) read from the map at the
    centre-3d (columns 4, 5: network-input pixels) truncated toward zero and clamped to the map; NaN and negative centres read index 0
    (include/y3d.h states the rule).  One HIP launch (`y3d_rows_depth_from_map`), capturable.  Inputs of another float dtype or strided
    views are taken through a float32 contiguous copy; the inputs are left as they are."""
    if not (torch.is_tensor(rows) and torch.is_tensor(depth_maps)) or rows.dim() != 3 or depth_maps.dim() != 3 or rows.shape[0] != depth_maps.shape[0]:
        raise Y3DError(f"depth_from_map: expected rows (B, K, C) and depth maps (B, Hm, Wm), got {tuple(getattr(rows, 'shape', ()))} / "
                       f"{tuple(getattr(depth_maps, 'shape', ()))}")
    if rows.device.type != "cuda" or depth_maps.device != rows.device:
        raise Y3DError("depth_from_map needs the rows and the depth maps on one HIP device (no host fallback)")
    if not (rows.is_floating_point() and depth_maps.is_floating_point()):
        raise Y3DError("depth_from_map: rows and depth maps must be floating point")
    R, D = rows.detach().float().contiguous(), depth_maps.detach().float().contiguous()
    out = torch.empty_like(R)
    B, K, C = R.shape
    lib().rows_depth_from_map(R.data_ptr(), B, K, C, D.data_ptr(), D.shape[1], D.shape[2], out.data_ptr(), ops.stream())
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# f3: image side of the input pipeline (data/datasets/kitti.py:132-206) on the device
# ------------------------------------------------------------------------------------------------------------------------------
def get_affine_transform(center, scale, output_size, inv=False):
    """kitti_utils.py:423-464 (rot = 0, shift = 0, as kitti.py:192 calls it): the crop's affine map, host side (six numbers per image).
    center (2,), scale = crop size (2,) or scalar, output_size (W, H) -> trans (2, 3) float64 [, trans_inv]"""
    import numpy as np
    center = np.asarray(center, np.float64)
    scale = np.asarray(scale, np.float64) if np.ndim(scale) else np.array([scale, scale], np.float64)
    src, dst = np.zeros((3, 2), np.float32), np.zeros((3, 2), np.float32)
    src[0] = center
    src[1] = center + np.array([0, scale[0] * -0.5])
    dst[0] = [output_size[0] * 0.5, output_size[1] * 0.5]
    dst[1] = np.array([output_size[0] * 0.5, output_size[1] * 0.5], np.float32) + np.array([0, output_size[0] * -0.5], np.float32)
    for p in (src, dst):  # third point: the right-angle companion (kitti_utils.py get_3rd_point)
        d = p[0] - p[1]
        p[2] = p[1] + np.array([-d[1], d[0]], np.float32)

    def solve(a, b):  # cv2.getAffineTransform: the exact map through three point pairs
        return np.linalg.solve(np.hstack((a.astype(np.float64), np.ones((3, 1)))), b.astype(np.float64)).T.copy()

    trans = solve(src, dst)
    return (trans, solve(dst, src)) if inv else trans


def affine_transform(pt, t):
    """kitti_utils.py:467-470: a point through the 2x3 map (labels: box corners, projected 3D centre)"""
    import numpy as np
    return np.dot(t, np.array([pt[0], pt[1], 1.0], dtype=np.float32).T)[:2]


def augment_images(imgs, partners, flips, trans_inv, out_wh, mode="float"):
    """The image work of `KITTIDataset.__getitem__` for a batch, one HIP launch: `imgs[b]` (H, W, 3) uint8 RGB device tensors as
    decoded, `partners[b]` the mixup partner or None (kitti.py:160-189), `flips[b]` bool (:147-149), `trans_inv[b]` the (2, 3) crop
    matrix (:192), `out_wh` = the dataset's resolution (W, H).
    mode "float": (B, 3, H, W) float32 in [0, 1] — the reference's `img` tensor, bit for bit; mode "uint8": (B, H, W, 3) uint8, which
    the stem consumes directly (the /255 and the layout change happen in `y3d_stem_im2col_u8`)."""
    import numpy as np
    B = len(imgs)
    if B == 0 or any((not t.is_cuda) or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 for t in imgs):
        raise Y3DError("augment_images: images must be (H, W, 3) uint8 tensors on a HIP device")
    dev = imgs[0].device
    imgs = [t.contiguous() for t in imgs]
    parts = [None if q is None else q.contiguous() for q in partners]
    for t, q in zip(imgs, parts):
        if q is not None and (q.shape != t.shape or q.dtype != torch.uint8 or not q.is_cuda):
            raise Y3DError("augment_images: a mixup partner must match its image (the reference mixes equal-sized frames only, kitti.py:176)")
    W, H = int(out_wh[0]), int(out_wh[1])
    src = torch.tensor([t.data_ptr() for t in imgs], dtype=torch.int64).to(dev)
    src2 = torch.tensor([0 if q is None else q.data_ptr() for q in parts], dtype=torch.int64).to(dev) if any(q is not None for q in parts) else None
    hw = torch.tensor([[t.shape[0], t.shape[1]] for t in imgs], dtype=torch.int32).to(dev)
    fl = torch.tensor([int(bool(f)) for f in flips], dtype=torch.int32).to(dev)
    ti = torch.tensor(np.stack([np.asarray(t, np.float64).reshape(6) for t in trans_inv]), dtype=torch.float64).to(dev)
    if mode == "float":
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
    elif mode == "uint8":
        out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
    else:
        raise ValueError("mode must be 'float' or 'uint8'")
    lib().kitti_image_aug(src.data_ptr(), src2.data_ptr() if src2 is not None else None, hw.data_ptr(), fl.data_ptr(), ti.data_ptr(), B, H, W,
                          0 if mode == "float" else 1, out.data_ptr(), ops.stream())
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# f3: label side of the input pipeline (data/datasets/kitti.py:208-405) and collate_fn (:579-599) on the device
# ------------------------------------------------------------------------------------------------------------------------------
CLASS_IDS = {"Car": 0, "Pedestrian": 1, "Cyclist": 2}  # kitti.py:24, the writelist
RESOLUTION = (1280, 384)  # W, H (kitti.py:25)
MAX_OBJS = 50  # kitti.py:22
PER_BOX = ("cls", "bboxes", "center_2d", "size_2d", "center_3d", "size_3d", "depth", "heading_bin", "heading_res", "batch_idx")
_REC_W = 16
# the data-pipeline hyper-parameters of cfg/default.yaml the dataset reads (kitti.py:61-70)
DATA_ARGS = dict(fliplr=0.5, random_crop=0.5, mixup=0.5, min_scale=0.8, max_scale=1.2, translate=0.1, min_depth_threshold=1,
                 max_depth_threshold=120, cam_dis=False, load_depth_maps=False)


def data_args(**over):
    """DATA_ARGS with overrides, as the attribute namespace build_batch / sample_augment read"""
    from types import SimpleNamespace
    return SimpleNamespace(**dict(DATA_ARGS, **over))


# ------------------------------------------------------------------------------------------------------------------------------
# foreground depth maps (`load_depth_maps`, data/datasets/kitti.py:54-56, 87-90, 143-145, 170-201, 286-287, 384-385, 409-417)
# ------------------------------------------------------------------------------------------------------------------------------
LINE_SLOTS = 64  # label lines per source in the per-line depth table (max_objs <= 64)


def seg_path(data_dir, idx):
    """the instance segmentation mask of frame `idx` of the split directory `data_dir` (<root>/training): under
    <root>/deepseg/training/image_2 when that directory exists, else next to the images (kitti.py:54-56)"""
    import os
    deep = os.path.join(os.path.dirname(os.path.abspath(data_dir)), "deepseg", "training", "image_2")
    return os.path.join(deep if os.path.exists(deep) else os.path.join(data_dir, "image_2"), f"{int(idx):06d}_seg.png")


def read_seg(path, with_wide=False):
    """A segmentation mask file -> (H, W) uint8: a pixel is the label-file line index of its object.  The file is read unchanged
    (kitti.py:87-90, cv2.imread(..., -1)) and must hold a single channel of 8 or 16 bits; ids above 255 are stored as 255 (only ids
    below max_objs can match a label line).  with_wide: -> (mask, whether the file holds 16 bits): Pillow warps a 16-bit image by
    another code path than an 8-bit one, so the depth map kernel needs to know."""
    import numpy as np
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("L", "I;16", "I;16L", "I;16B"):
            raise Y3DError(f"read_seg: {path} is a {im.mode} image; a mask has a single channel of 8 or 16 bits")
        px = np.array(im)
    if px.ndim != 2:
        raise Y3DError(f"read_seg: {path} decodes to {px.shape}; a mask has a single channel")
    px, wide = np.minimum(px, 255).astype(np.uint8), px.dtype.itemsize == 2
    return (px, wide) if with_wide else px


def _depth_map_launch(B, out_wh, max_depth, max_side, dev, **tables):
    """the launch of `y3d_kitti_depth_map` shared by augment_depth_maps (mask pointers) and DeviceSplit (the mask arena)"""
    W, H = int(out_wh[0]), int(out_wh[1])
    out = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    xy = torch.empty(B, W + H, dtype=torch.int32, device=dev)
    ptr = lambda k: tables[k].data_ptr() if tables.get(k) is not None else None
    lib().kitti_depth_map(ptr("mask"), ptr("mask2"), ptr("arena"), ptr("mask_off"), ptr("draws"), int(tables.get("draw_w", 0)), ptr("wide"),
                          ptr("hw"), ptr("flip"), ptr("trans_inv"), ptr("line_depth"), B, H, W, int(max_side), float(max_depth), xy.data_ptr(),
                          out.data_ptr(), ops.stream())
    return out


def augment_depth_maps(masks, partners, flips, trans_inv, line_depth, out_wh=RESOLUTION, max_depth=120.0, wide=None):
    """The foreground depth maps of a batch on the device (csrc/kitti_depth_map.hip), the counterpart of augment_images: `masks[b]` an
    (h, w) uint8 device tensor (read_seg), `partners[b]` the mixup partner's or None, `flips[b]`, `trans_inv[b]` the (2, 3) crop matrix
    of the image, `line_depth` (B, 2, 64) float32 on the device (encode_labels(..., depths=True): the depth each own / partner label
    line paints, +inf for none).  Every mask is mirrored and warped as Pillow's Image.transform(AFFINE, NEAREST, fillcolor=51) does,
    bit for bit; a pixel takes the smaller depth of its two objects, 0 where there is none or it exceeds max_depth.  wide: None (every
    mask came from an 8-bit file) or per image (own, partner) flags of the masks read from 16-bit files (read_seg(..., with_wide=True)):
    Pillow warps those by its generic double-precision path.  -> (B, H, W) float32 at out_wh = (W, H)."""
    import numpy as np
    B = len(masks)
    if B == 0 or any((not t.is_cuda) or t.dtype != torch.uint8 or t.dim() != 2 for t in masks):
        raise Y3DError("augment_depth_maps: masks must be (h, w) uint8 tensors on a HIP device")
    dev = masks[0].device
    masks = [t.contiguous() for t in masks]
    parts = [None if q is None else q.contiguous() for q in partners]
    for t, q in zip(masks, parts):
        if q is not None and (q.shape != t.shape or q.dtype != torch.uint8 or not q.is_cuda):
            raise Y3DError("augment_depth_maps: a mixup partner's mask must match its image's mask")
    if not (torch.is_tensor(line_depth) and line_depth.is_cuda and line_depth.dtype == torch.float32
            and tuple(line_depth.shape) == (B, 2, LINE_SLOTS) and line_depth.is_contiguous()):
        raise Y3DError(f"augment_depth_maps: line_depth must be a contiguous ({B}, 2, {LINE_SLOTS}) float32 tensor on a HIP device")
    if len(parts) != B or len(flips) != B or len(trans_inv) != B or (wide is not None and len(wide) != B):
        raise Y3DError("augment_depth_maps: partners, flips, trans_inv and wide need one entry per mask")
    wd = None if wide is None else torch.tensor([[int(bool(a)), int(bool(b))] for a, b in wide], dtype=torch.uint8).to(dev)
    mask = torch.tensor([t.data_ptr() for t in masks], dtype=torch.int64).to(dev)
    mask2 = torch.tensor([0 if q is None else q.data_ptr() for q in parts], dtype=torch.int64).to(dev) if any(q is not None for q in parts) else None
    hw = torch.tensor([[t.shape[0], t.shape[1]] for t in masks], dtype=torch.int32).to(dev)
    fl = torch.tensor([int(bool(f)) for f in flips], dtype=torch.int32).to(dev)
    ti = torch.tensor(np.stack([np.asarray(t, np.float64).reshape(6) for t in trans_inv]), dtype=torch.float64).to(dev)
    return _depth_map_launch(B, out_wh, max_depth, max(max(t.shape) for t in masks), dev, mask=mask, mask2=mask2, hw=hw, flip=fl, trans_inv=ti,
                             line_depth=line_depth, wide=wd)


def _level(box, trunc, occ):
    """kitti_utils.py Object3d.get_obj_level, from the label's own box"""
    height = float(box[3]) - float(box[1]) + 1
    if trunc == -1:
        return "DontCare"
    if height >= 40 and trunc <= 0.15 and occ <= 0:
        return "Easy"
    if height >= 25 and trunc <= 0.3 and occ <= 1:
        return "Moderate"
    if height >= 25 and trunc <= 0.5 and occ <= 2:
        return "Hard"
    return "UnKnown"


def read_label(path):
    """A KITTI label file -> dict of per-line arrays in the reference's parse dtypes (kitti_utils.py Object3d): `type`, `level` (lists of
    str), `truncation`, `occlusion`, `alpha`, `h`, `w`, `l`, `ry` float64, `box2d` (n, 4) float32, `pos` (n, 3) float32"""
    import numpy as np
    cols = [ln.strip().split(" ") for ln in open(path).read().splitlines() if ln.strip()]
    f = lambda c: np.array([float(r[c]) for r in cols], np.float64)
    lab = {"type": [r[0] for r in cols], "truncation": f(1), "occlusion": f(2), "alpha": f(3), "h": f(8), "w": f(9), "l": f(10), "ry": f(14),
           "box2d": np.array([[float(v) for v in r[4:8]] for r in cols], np.float32).reshape(-1, 4),
           "pos": np.array([[float(v) for v in r[11:14]] for r in cols], np.float32).reshape(-1, 3)}
    lab["level"] = [_level(b, t, o) for b, t, o in zip(lab["box2d"], lab["truncation"], lab["occlusion"])]
    return lab


def read_calib(path):
    """A KITTI calibration file -> P2 (3, 4) float32 (its third line, kitti_utils.py get_calib_from_file)"""
    import numpy as np
    line = open(path).read().splitlines()[2]
    return np.array(line.strip().split(" ")[1:], np.float32).reshape(3, 4)


def calib_params(P2):
    """(cu, cv, fu, fv, tx, ty) of a float32 P2 as the reference's Calibration holds them (tx, ty divided in float32)"""
    import numpy as np
    P = np.asarray(P2, np.float32)
    return (float(P[0, 2]), float(P[1, 2]), float(P[0, 0]), float(P[1, 1]), float(P[0, 3] / -P[0, 0]), float(P[1, 3] / -P[1, 1]))


def _flip_fit(cam, W, H, p23):
    """flip_calib's fit for the intrinsics cam = (cu, cv, fu, fv, tx, ty) of a W x H image; p23 = P2[2, 3] -> P2 (3, 4) float32"""
    import numpy as np
    cu, cv, fu, fv, tx, ty = cam
    u = np.tile(np.linspace(0.0, W, 4), 2)
    v = np.repeat(np.linspace(0.0, H, 2), 4)
    z = np.linspace(2.0, 78.0, 8)
    x, y = ((u - cu) * z) / fu + tx, ((v - cv) * z) / fv + ty
    x, u = -x, W - u
    # unknowns (f, c_u, c_v, t_u, t_v, d): u * (z + d) = f x + c_u z + t_u and v * (z + d) = f y + c_v z + t_v
    one, nil = np.ones(8), np.zeros(8)
    A = np.concatenate([np.stack([x, z, nil, one, nil, -u], 1), np.stack([y, nil, z, nil, one, -v], 1)])
    rhs = np.concatenate([u * z, v * z])
    f, c_u, c_v, t_u, t_v, _ = np.linalg.lstsq(A, rhs, rcond=None)[0]
    out = np.zeros((3, 4), np.float32)
    out[0] = (f, 0.0, c_u, t_u)
    out[1] = (0.0, f, c_v, t_v)
    out[2, 3] = p23
    return out


def flip_calib(P2, img_size):
    """The projection of the mirrored image (kitti_utils.py Calibration.flip): eight pixels of a 4 x 2 grid over the image, at depths
    2 .. 78, are lifted to 3D with the float32 calibration, mirrored (x -> -x, u -> W - u), and a pinhole camera with fu = fv is fitted to
    them by least squares in float64.  -> P2 (3, 4) float32; as in the reference, its third row is (0, 0, 0, P2[2, 3])."""
    import numpy as np
    return _flip_fit(calib_params(P2), float(img_size[0]), float(img_size[1]), np.asarray(P2, np.float32)[2, 3])


def sample_augment(n, items, frame_info, args, mode="train", max_objs=MAX_OBJS, resolution=RESOLUTION):
    """The random decisions of `KITTIDataset.__getitem__` (kitti.py:132-189) for dataset positions `items`, drawn from np.random in the
    reference's order, so a seeded run decides as the reference with workers=0: mixup random(), flip random(), crop random(), the crop's
    three randn (scale, x shift, y shift) only when cropping, then up to 50 randint(n) partner tries.  A partner has the primary's
    (cu, cv, fu, fv), its size (when frame_info gives one) and fewer than max_objs label lines together with it.
    frame_info(position) -> (cam (cu, cv, fu, fv) of its unflipped float32 P2, label line count, (W, H) or None); n = dataset length.
    -> one dict per item: mixed, flip, crop (bool), scale, center (2,), crop_size (2,), partner (position or -1), trans, trans_inv."""
    import numpy as np
    aug = mode in ("train", "trainval")
    out = []
    for item in items:
        cam, nl, size = frame_info(item)
        img_size = np.asarray(size, np.int64)
        center, crop_size, scale = img_size / 2, img_size, 1.0
        want_mix = flip = crop = False
        if aug:
            want_mix = np.random.random() < 0.5 and bool(args.mixup)
            flip = np.random.random() < args.fliplr
            if np.random.random() < args.random_crop:
                crop = True
                half, mid = (args.max_scale - args.min_scale) / 2, (args.max_scale + args.min_scale) / 2
                scale = float(np.clip(np.random.randn() * half + mid, args.min_scale, args.max_scale))
                crop_size = img_size * scale
                t = args.translate
                center = center + np.array([img_size[0] * np.clip(np.random.randn() * t, -2 * t, 2 * t),
                                            img_size[1] * np.clip(np.random.randn() * t, -2 * t, 2 * t)])
        partner = -1
        if want_mix:
            for _ in range(50):
                pos = int(np.random.randint(n))
                cam2, nl2, size2 = frame_info(pos)
                if tuple(cam2) == tuple(cam) and (size2 is None or tuple(size2) == tuple(size)) and nl + nl2 < max_objs:
                    partner = pos
                    break
        trans, trans_inv = get_affine_transform(center, crop_size, resolution, inv=True)
        out.append(dict(mixed=partner >= 0, flip=bool(flip), crop=crop, scale=scale, center=np.asarray(center, np.float64),
                        crop_size=np.asarray(crop_size, np.float64), partner=partner, trans=trans, trans_inv=trans_inv))
    return out


def label_records(lab):
    """read_label's dict -> (n, 16) float64 records of y3d_kitti_encode_labels"""
    import numpy as np
    n = len(lab["type"])
    r = np.zeros((n, _REC_W), np.float64)
    r[:, 0] = [CLASS_IDS.get(t, -1) for t in lab["type"]]
    r[:, 1], r[:, 2] = lab["truncation"], lab["occlusion"]
    r[:, 3:7] = lab["box2d"]
    r[:, 7], r[:, 8], r[:, 9] = lab["h"], lab["w"], lab["l"]
    r[:, 10:13] = lab["pos"]
    r[:, 13] = lab["ry"]
    return r


def _pack(items, partners, P2s, trans, flips, scales, img_sizes, device, source):
    """pack_labels of this module and of json3d.  source = (records, rec_w, p2_dtype, mean_size): `records(item)` -> the (n, rec_w)
    float64 records of one image, the dtype the projections are rounded to on their way into `img_f`, the class mean sizes."""
    import numpy as np
    records, rec_w, p2_dtype, mean_size = source
    if torch.device(device).type != "cuda":
        raise Y3DError("pack_labels: the label encoder runs on a HIP device (no host fallback)")
    B = len(items)
    recs, img_i, img_f, row = [], np.zeros((B, 7), np.int32), np.zeros((B, 19), np.float64), 0
    for b in range(B):
        r0 = records(items[b])
        r1 = records(partners[b]) if partners[b] is not None else np.zeros((0, rec_w))
        img_i[b] = (row, len(r0), row + len(r0), len(r1), int(bool(flips[b])), int(img_sizes[b][0]), int(img_sizes[b][1]))
        img_f[b, :12] = np.asarray(P2s[b], p2_dtype).reshape(12)
        img_f[b, 12:18] = np.asarray(trans[b], np.float64).reshape(6)
        img_f[b, 18] = float(scales[b])
        recs += [r0, r1]
        row += len(r0) + len(r1)
    rec = np.concatenate(recs) if row else np.zeros((1, rec_w))
    return {"rec": upload(rec, device, torch.float64), "img_i": upload(img_i, device, torch.int32), "img_f": upload(img_f, device, torch.float64),
            "mean_size": upload(np.asarray(mean_size, np.float64).reshape(-1, 3), device, torch.float64)}


def pack_labels(labels, partners, P2s, trans, flips, scales, img_sizes, device, cls_mean_size=CLS_MEAN_SIZE):
    """Host side of encode_labels: B images' read_label dicts (partners[b]: the mixup partner's, or None), their P2 (flipped when
    flips[b]: flip_calib), crop matrices `trans` (2, 3), crop scales and original (W, H) -> dict of device tensors (one upload each)"""
    return _pack(labels, partners, P2s, trans, flips, scales, img_sizes, device, (label_records, _REC_W, "float32", cls_mean_size))


def _label_outputs(B, max_objs, dev):
    """the thirteen tensors of encode_labels' static layout, unwritten"""
    n = B * max_objs
    e = lambda *s, dt: torch.empty(*s, dtype=dt, device=dev)
    return {"cls": e(n, 1, dt=torch.int64), "bboxes": e(n, 4, dt=torch.float64), "center_2d": e(n, 2, dt=torch.float32),
            "size_2d": e(n, 2, dt=torch.float32), "center_3d": e(n, 2, dt=torch.float64), "size_3d": e(n, 3, dt=torch.float64),
            "depth": e(n, dt=torch.float64), "heading_bin": e(n, dt=torch.int64), "heading_res": e(n, dt=torch.float64),
            "batch_idx": e(n, dt=torch.float32), "counts": e(B, dt=torch.int32), "calib": e(B, 6, dt=torch.float64),
            "ratio_pad": e(B, 2, 2, dt=torch.float64)}


def encode_labels(packed, out_wh=RESOLUTION, min_depth=1.0, max_depth=120.0, use_camera_dis=False, max_objs=MAX_OBJS, depths=False):
    """The label encoding of `KITTIDataset.__getitem__` + `collate_fn` for a packed batch (pack_labels), one HIP launch, no host
    synchronisation (capturable).  -> dict of the per-box keys in a static layout: image b owns rows [b * max_objs, b * max_objs + count);
    unused rows have batch_idx = -1 (skipped by pad_targets) and zeros elsewhere; plus `counts` (B,) int32, `calib` (B, 6) float64,
    `ratio_pad` (B, 2, 2) float64.  depths: the same launch also writes `line_depth` (B, 2, 64) float32, the depth every own /
    partner label line paints into the foreground depth map (+inf: dropped or absent), what `augment_depth_maps` takes."""
    img_i = packed["img_i"]
    if not img_i.is_cuda or any(not packed[k].is_cuda for k in ("rec", "img_f", "mean_size")):
        raise Y3DError("encode_labels: the packed labels must live on a HIP device (no host fallback)")
    B = img_i.shape[0]
    o = _label_outputs(B, max_objs, img_i.device)
    ms = packed["mean_size"]
    a = (packed["rec"].data_ptr(), img_i.data_ptr(), packed["img_f"].data_ptr(), B, int(out_wh[0]), int(out_wh[1]), float(min_depth),
         float(max_depth), int(bool(use_camera_dis)), ms.data_ptr(), ms.shape[0], int(max_objs), *[o[k].data_ptr() for k in PER_BOX],
         o["counts"].data_ptr(), o["calib"].data_ptr(), o["ratio_pad"].data_ptr())
    if depths:
        o["line_depth"] = torch.empty(B, 2, LINE_SLOTS, dtype=torch.float32, device=img_i.device)
        lib().kitti_encode_labels_depths(*a, o["line_depth"].data_ptr(), ops.stream())
    else:
        lib().kitti_encode_labels(*a, ops.stream())
    return o


def compact_labels(static, counts, crops, use_camera_dis=False, max_objs=MAX_OBJS):
    """Static layout -> the ragged per-box tensors `collate_fn` returns, in its shapes and dtypes.  torch.cat promotes over every
    image's tensor: an image without boxes contributes a float64 (0,) tensor (bboxes: float32), an image's depth is float32 when it was
    neither cropped nor encoded as camera distance, heading_res and the 2D centre / size are float32.  counts: host ints (B,)."""
    return _compact(static, counts, crops, use_camera_dis, max_objs, {})


def _compact(static, counts, crops, use_camera_dis, max_objs, wider):
    """compact_labels of this module and of json3d.  wider: {key: dtype} of the per-box keys a dataset holds in a wider dtype"""
    B = len(counts)
    rows = torch.cat([torch.arange(b * max_objs, b * max_objs + int(c)) for b, c in enumerate(counts)]).to(static["cls"].device)
    total = int(sum(int(c) for c in counts))
    own = {"cls": torch.int64, "bboxes": torch.float64, "center_2d": torch.float32, "size_2d": torch.float32, "center_3d": torch.float64,
           "size_3d": torch.float64, "heading_bin": torch.int64, "heading_res": torch.float32, "batch_idx": torch.float32, **wider}
    out = {}
    for k in PER_BOX:
        dts = []
        for b in range(B):
            if k == "batch_idx":
                dts.append(torch.float32)
            elif int(counts[b]) == 0:
                dts.append(torch.float32 if k == "bboxes" else torch.float64)
            elif k == "depth":
                dts.append(torch.float64 if (crops[b] or use_camera_dis) else torch.float32)
            else:
                dts.append(own[k])
        dt = dts[0]
        for d in dts[1:]:
            dt = torch.promote_types(dt, d)
        v = static[k].index_select(0, rows).to(dt)
        out[k] = v if total else v.reshape(0)
    return out


_SPLITS = {}


def _split(root_or_split_file, mode):
    import os
    if os.path.isdir(root_or_split_file):
        split_file = os.path.join(root_or_split_file, "ImageSets", f"{mode}.txt")
    else:
        split_file = root_or_split_file
    root = os.path.dirname(os.path.dirname(os.path.abspath(split_file)))
    data = os.path.join(root, "testing" if mode == "test" else "training")
    ids = [int(s.strip()) for s in open(split_file).read().splitlines() if s.strip()]
    return data, ids


def _batch(img, lab, ids, sizes, draws, mean_size, mixed, compact, depth_map=None):
    """The dictionary every 3D builder returns (json3d's too): the images, encode_labels' `lab`, and per image its id, its original
    (W, H) and its draws.  compact: false for the per-box keys in the static layout, or counts (host ints) -> the ragged ones.
    depth_map: the KITTI builders' (B, H, W) float32 foreground depth maps under `load_depth_maps` (no key without)."""
    import numpy as np
    batch = {"img": img, "calib": lab["calib"],
             "info": [{"img_id": i, "img_size": np.array(s), "trans_inv": d["trans_inv"]} for i, s, d in zip(ids, sizes, draws)],
             "im_file": [f"{i:06d}.txt" for i in ids], "ori_shape": [np.array(s)[::-1] for s in sizes],
             "ratio_pad": lab["ratio_pad"], "mean_sizes": mean_size, "mixed": mixed, "counts": lab["counts"]}
    if compact:
        batch.update(compact(lab["counts"].tolist()))
        del batch["counts"]
    else:
        batch.update({k: lab[k] for k in PER_BOX})
    if depth_map is not None:
        batch["depth_map"] = depth_map
    return batch


def _resident_tail(split, plan, args, cam_dis, img_mode, resolution, encode, **packed):
    """What a resident split's `build_batch` launches behind its plan (json3d's too): the images of `img_mode` by `kitti_image_aug`
    from the plan's tables, and the labels by `encode` (this module's encode_labels or json3d's; packed: what its dict holds beyond
    the split's records and the plan's tables).  -> (img, lab)"""
    B, W, H = plan["img_i"].shape[0], int(resolution[0]), int(resolution[1])
    if img_mode == "float":
        img = torch.empty(B, 3, H, W, dtype=torch.float32, device=split.device)
    else:
        img = torch.empty(B, H, W, 3, dtype=torch.uint8, device=split.device)
    lib().kitti_image_aug(plan["src"].data_ptr(), plan["src2"].data_ptr(), plan["hw"].data_ptr(), plan["flip"].data_ptr(),
                          plan["trans_inv"].data_ptr(), B, H, W, 0 if img_mode == "float" else 1, img.data_ptr(), ops.stream())
    encode_kw = packed.pop("encode_kw", {})
    packed = dict(rec=split.rec, img_i=plan["img_i"], img_f=plan["img_f"], mean_size=split.mean_size, **packed)
    return img, encode(packed, resolution, args.min_depth_threshold, args.max_depth_threshold, cam_dis, MAX_OBJS, **encode_kw)


def build_batch(root_or_split_file, indices, args, device, mode="train", compact=False, img_mode="uint8", resolution=RESOLUTION):
    """`collate_fn([dataset[i] for i in indices])` of the reference's KITTIDataset (kitti.py:116-442, 579-599) with the image and label
    work on the device: PNGs (PIL), labels and calibrations are read on the host, the random decisions drawn (sample_augment), the
    images mixed / mirrored / cropped by augment_images and the labels encoded by encode_labels.  root_or_split_file: a split file
    (ImageSets/<split>.txt) or the KITTI root (then ImageSets/<mode>.txt).  -> every key collate_fn returns except ori_img and depth_map;
    the per-box keys in encode_labels' static layout, or with compact=True (one read-back of the counts) in collate_fn's ragged shapes.
    img_mode "uint8": (B, H, W, 3) uint8 for the stem; "float": the reference's (B, 3, H, W) float32.
    root_or_split_file may also be a `DeviceSplit`: the same batch from the split held on the device, without any file access."""
    import os
    import numpy as np
    from PIL import Image
    if isinstance(root_or_split_file, DeviceSplit):  # the split is resident on the device: no file is touched
        root_or_split_file.check_device(device)
        return root_or_split_file.build_batch(indices, args, mode=mode, compact=compact, img_mode=img_mode, resolution=resolution)
    depth = bool(getattr(args, "load_depth_maps", False))
    if torch.device(device).type != "cuda":
        raise Y3DError("build_batch: the batch is built on a HIP device (no host fallback)")
    if mode == "test":
        raise Y3DError("build_batch: the test split has no labels")
    data, ids = _split(root_or_split_file, mode)
    path = lambda sub, i, ext: os.path.join(data, sub, f"{i:06d}.{ext}")
    if depth:  # the batch's own masks before anything is decoded (a partner's once it is drawn)
        for pos in indices:
            if not os.path.exists(seg_path(data, ids[pos])):
                raise Y3DError(f"build_batch: load_depth_maps: frame {ids[pos]:06d} has no segmentation mask ({seg_path(data, ids[pos])})")
    calib_cache, label_cache = {}, {}

    def calib(i):
        if i not in calib_cache:
            calib_cache[i] = read_calib(path("calib", i, "txt"))
        return calib_cache[i]

    def label(i):
        if i not in label_cache:
            label_cache[i] = read_label(path("label_2", i, "txt"))
        return label_cache[i]

    sizes = {}

    def frame_info(pos):
        i = ids[pos]
        P = calib(i)
        return (P[0, 2], P[1, 2], P[0, 0], P[1, 1]), len(label(i)["type"]), sizes.get(pos)

    frames = []
    for pos in indices:
        im = Image.open(path("image_2", ids[pos], "png"))
        sizes[pos] = im.size
        frames.append(im)
    draws = sample_augment(len(ids), indices, frame_info, args, mode, MAX_OBJS, resolution)
    to_dev = lambda im: torch.from_numpy(np.array(im.convert("RGB"))).to(device)
    imgs = [to_dev(im) for im in frames]
    parts = [to_dev(Image.open(path("image_2", ids[d["partner"]], "png"))) if d["mixed"] else None for d in draws]
    img = augment_images(imgs, parts, [d["flip"] for d in draws], [d["trans_inv"] for d in draws], resolution,
                         mode="float" if img_mode == "float" else "uint8")
    P2s, labels, partners = [], [], []
    for pos, d, im in zip(indices, draws, frames):
        P = calib(ids[pos])
        P2s.append(flip_calib(P, im.size) if d["flip"] else P)
        labels.append(label(ids[pos]))
        partners.append(label(ids[d["partner"]]) if d["mixed"] else None)
    packed = pack_labels(labels, partners, P2s, [d["trans"] for d in draws], [d["flip"] for d in draws], [d["scale"] for d in draws],
                         [im.size for im in frames], device)
    lab = encode_labels(packed, resolution, args.min_depth_threshold, args.max_depth_threshold, bool(args.cam_dis), MAX_OBJS, depths=depth)
    mixed = torch.tensor([int(d["mixed"]) for d in draws], dtype=torch.uint8).to(device)
    depth_map = None
    if depth:  # the masks of the frames and of their partners (kitti.py:125-126, 170-171), warped with the images' matrices
        def mask(pos, size):
            f = seg_path(data, ids[pos])
            if not os.path.exists(f):
                raise Y3DError(f"build_batch: load_depth_maps: frame {ids[pos]:06d} has no segmentation mask ({f})")
            px, wide = read_seg(f, with_wide=True)
            if px.shape != (size[1], size[0]):
                raise Y3DError(f"build_batch: load_depth_maps: the mask of frame {ids[pos]:06d} is {px.shape[1]} x {px.shape[0]}, "
                               f"its image {size[0]} x {size[1]}")
            return torch.from_numpy(px).to(device), wide

        masks = [mask(pos, im.size) for pos, im in zip(indices, frames)]
        pmasks = [mask(d["partner"], im.size) if d["mixed"] else (None, False) for d, im in zip(draws, frames)]
        depth_map = augment_depth_maps([m for m, _ in masks], [m for m, _ in pmasks], [d["flip"] for d in draws],
                                       [d["trans_inv"] for d in draws], lab["line_depth"], resolution, args.max_depth_threshold,
                                       wide=[(a[1], b[1]) for a, b in zip(masks, pmasks)])
    return _batch(img, lab, [ids[p] for p in indices], [im.size for im in frames], draws, packed["mean_size"], mixed,
                  compact and (lambda counts: compact_labels(lab, counts, [d["crop"] for d in draws], bool(args.cam_dis))), depth_map)


# ------------------------------------------------------------------------------------------------------------------------------
# the split resident on the device: decoded once, then a batch is the draws, one small upload and three launches
# ------------------------------------------------------------------------------------------------------------------------------
_DRAW_W = 16  # a row of the draw table: position, partner (-1: none), flip, scale, trans (6), trans_inv (6)
PLAN_TABLES = (("src", torch.int64, ()), ("src2", torch.int64, ()), ("hw", torch.int32, (2,)), ("flip", torch.int32, ()),
         ("trans_inv", torch.float64, (6,)), ("img_i", torch.int32, (7,)), ("img_f", torch.float64, (19,)), ("mixed", torch.uint8, ()))


def draw_table(indices, draws):
    """sample_augment's draws for dataset positions `indices` -> the (B, 16) float64 draw table of `y3d_kitti_plan_batch`, rows
    [position, partner or -1, flip, scale, trans (6), trans_inv (6)]"""
    import numpy as np
    table = np.empty((len(indices), _DRAW_W), np.float64)
    for row, p, d in zip(table, indices, draws):
        row[:4] = (p, d["partner"], d["flip"], d["scale"])
        row[4:10], row[10:] = d["trans"].reshape(6), d["trans_inv"].reshape(6)
    return table


def plan_batch(split, draws, draws_dev=None, out=None):
    """The per-image tables of `y3d_kitti_image_aug` and `y3d_kitti_encode_labels` for a table of draws over a DeviceSplit, one HIP
    launch (`y3d_kitti_plan_batch`).  draws: (B, 16) float64 on the host (numpy or tensor), rows [position, partner or -1, flip, scale,
    trans (6), trans_inv (6)]; draws_dev: the same table on the device (uploaded here when None).  Positions and partners outside the
    split are refused from the host table.  out: optionally the eight output tensors (at least B rows each; the first B are written).
    -> dict src, src2 (B) int64, hw (B, 2) int32, flip (B) int32, trans_inv (B, 6) float64, img_i (B, 7) int32, img_f (B, 19) float64,
    mixed (B) uint8."""
    host, draws_dev, out = check_plan(draws, _DRAW_W, split.device, PLAN_TABLES, draws_dev, out)
    lib().kitti_plan_batch(split.img_off.data_ptr(), split.frame_hw.data_ptr(), split.rec_span.data_ptr(), split.P2.data_ptr(), len(split),
                           split.arena.data_ptr(), host.data_ptr(), draws_dev.data_ptr(), host.shape[0],
                           *[out[k].data_ptr() for k, _, _ in PLAN_TABLES], ops.stream())
    return out


class DeviceSplit(ResidentSplit):
    """A KITTI split decoded once and held on the device: `DeviceSplit(root_or_split_file, mode)` resolves the split as build_batch does,
    checks the bytes it needs against `max_bytes` (default: half of the device's free memory) from the PNG headers alone, then decodes
    every frame with `min(workers, 16)` threads into one uint8 arena (`arena`: each frame (H, W, 3) RGB at a multiple of 16 bytes,
    uploaded in large pinned chunks) and uploads the frame tables, indexed by dataset position: `img_off` (N) int64, `frame_hw` (N, 2)
    int32 (H, W), `rec` (R, 16) float64 = label_records of every frame in order, `rec_span` (N, 2) int32 (first row, lines), `P2`
    (N, 2, 12) float32 (as read; flip_calib of it), `mean_size`.  What sample_augment's frame_info needs stays on the host as well.

    `build_batch` then returns what `build_batch(path, ...)` returns, bit for bit, without touching a file: the draws, one non-blocking
    upload of the draw table from a ring of pinned buffers and three launches (plan_batch, the image augmentation, the label encoder).
    `frame_info` knows every frame's true size, as the reference's dataset does; the path-based builder knows those of the batch's own
    frames only, so the two draw the same mixup partners when frames that share a calibration share a size."""

    def __init__(self, root_or_split_file, mode="train", device="cuda", max_bytes=None, workers=8, load_depth_maps=False):
        import os
        import numpy as np
        from concurrent.futures import ThreadPoolExecutor
        from PIL import Image
        dev = self._accept(device, mode, workers)
        self.data, self.ids = _split(root_or_split_file, mode)
        path = lambda sub, i, ext: os.path.join(self.data, sub, f"{i:06d}.{ext}")
        # sizes from the PNG headers, the budget before anything is decoded or allocated
        hw = self._sizes([path("image_2", i, "png") for i in self.ids])
        self.load_depth_maps = bool(load_depth_maps)
        if self.load_depth_maps:  # a second arena, one byte per pixel of every frame's mask: both arenas share the budget
            px = np.asarray(hw, np.int64).reshape(-1, 2).prod(1)
            self._mask_padded = (px + ALIGN - 1) // ALIGN * ALIGN
            self.mask_offsets = np.concatenate(([0], np.cumsum(self._mask_padded)[:-1])).astype(np.int64)
            self.mask_nbytes = int(self._mask_padded.sum())
            frames = int(((px * 3 + ALIGN - 1) // ALIGN * ALIGN).sum())
            allowed = int(max_bytes) if max_bytes is not None else torch.cuda.mem_get_info(dev)[0] // 2
            if frames + self.mask_nbytes > allowed:
                raise Y3DError(f"DeviceSplit: the {len(hw)} decoded frames and their masks need {frames} + {self.mask_nbytes} bytes, "
                               f"{allowed} bytes are allowed (max_bytes)")
            missing = [i for i in self.ids if not os.path.exists(seg_path(self.data, i))]
            if missing:
                raise Y3DError(f"DeviceSplit: load_depth_maps: frame {missing[0]:06d} has no segmentation mask "
                               f"({seg_path(self.data, missing[0])}); {len(missing)} of {len(self.ids)} frames lack one")
        self._layout(dev, hw, max_bytes)

        # labels and calibrations, both projections of every frame
        def tables(pos):
            P = read_calib(path("calib", self.ids[pos], "txt"))
            return label_records(read_label(path("label_2", self.ids[pos], "txt"))), P, flip_calib(P, self.wh[pos])

        with ThreadPoolExecutor(max_workers=min(int(workers), 16)) as pool:
            recs, self.P2_host, flipped = zip(*pool.map(tables, range(len(self.ids))))
        self.n_lines = [len(r) for r in recs]
        self.cam = [(float(P[0, 2]), float(P[1, 2]), float(P[0, 0]), float(P[1, 1])) for P in self.P2_host]
        self.rec = upload(np.concatenate(recs) if sum(self.n_lines) else np.zeros((1, _REC_W)), dev, torch.float64)
        self.P2 = upload(np.stack([np.stack((P.reshape(12), F.reshape(12))) for P, F in zip(self.P2_host, flipped)]).astype(np.float32), dev,
                         torch.float32)
        self.mean_size = upload(np.asarray(CLS_MEAN_SIZE, np.float64).reshape(-1, 3), dev, torch.float64)

        def decode(pos):
            with Image.open(path("image_2", self.ids[pos], "png")) as im:
                return np.array(im.convert("RGB"))

        self._fill(span_table(self.n_lines), decode, lambda pos: f"frame {self.ids[pos]:06d}", workers, _DRAW_W)
        if self.load_depth_maps:
            self._fill_masks(workers)

    def _fill_masks(self, workers):
        """every frame's mask (read_seg) into `mask_arena`, one byte per pixel at `mask_offsets` (multiples of 16), `mask_off`, the
        offsets on the device, and `mask_wide` (N) uint8, the frames whose mask file holds 16 bits; a mask of another size than its
        frame is refused"""
        import numpy as np
        from concurrent.futures import ThreadPoolExecutor
        wide = np.zeros(len(self.ids), np.uint8)

        def decode(pos):
            px, wide[pos] = read_seg(seg_path(self.data, self.ids[pos]), with_wide=True)
            h, w = int(self._hw[pos][0]), int(self._hw[pos][1])
            if px.shape != (h, w):
                raise Y3DError(f"DeviceSplit: load_depth_maps: the mask of frame {self.ids[pos]:06d} is {px.shape[1]} x {px.shape[0]}, "
                               f"its image {w} x {h}")
            return px

        self.mask_arena = torch.empty(self.mask_nbytes, dtype=torch.uint8, device=self.device)
        self.mask_off = upload(self.mask_offsets, self.device, torch.int64)
        with ThreadPoolExecutor(max_workers=min(int(workers), 16)) as pool:
            fill_arena(self.mask_arena, self.mask_offsets, self._mask_padded, decode, pool, self.CHUNK)
        self.mask_wide = upload(wide, self.device, torch.uint8)

    def __len__(self):
        return len(self.ids)

    def frame_info(self, pos):
        """sample_augment's frame_info: ((cu, cv, fu, fv), label lines, (W, H)), the true size for every position"""
        return self.cam[pos], self.n_lines[pos], self.wh[pos]

    def build_batch(self, indices, args, mode="train", compact=False, img_mode="uint8", resolution=RESOLUTION):
        """`build_batch(path, indices, args, device, ...)` from the resident split: the same dictionary, bit for bit.  With compact=False
        nothing here waits for the device (but a ring buffer still in flight) and no file is opened."""
        depth = bool(getattr(args, "load_depth_maps", False))
        if depth and not self.load_depth_maps:
            raise Y3DError("build_batch: depth maps (load_depth_maps): this resident split holds no segmentation masks; build it with "
                           "DeviceSplit(..., load_depth_maps=True)")
        if mode == "test":
            raise Y3DError("build_batch: the test split has no labels")
        indices = [int(i) for i in indices]
        N, B = len(self), len(indices)
        if B < 1 or any(not 0 <= p < N for p in indices):
            raise Y3DError(f"build_batch: {B} positions, all must lie in [0, {N})")
        draws = sample_augment(N, indices, self.frame_info, args, mode, MAX_OBJS, resolution)
        for pos, d in zip(indices, draws):
            if d["mixed"] and self.wh[d["partner"]] != self.wh[pos]:
                raise Y3DError(f"build_batch: mixup partner {d['partner']} of position {pos} has another size")
        cam_dis = bool(args.cam_dis)
        with torch.cuda.device(self.device):
            host, dev = self._ring.upload(draw_table(indices, draws))
            plan = plan_batch(self, host, dev)
            img, lab = _resident_tail(self, plan, args, cam_dis, img_mode, resolution, encode_labels,
                                      **({"encode_kw": {"depths": True}} if depth else {}))
            depth_map = None
            if depth:  # the masks' addresses come from the arena offsets and the draw table's position / partner columns
                depth_map = _depth_map_launch(B, resolution, args.max_depth_threshold, int(self._hw.max()), self.device, arena=self.mask_arena,
                                              mask_off=self.mask_off, wide=self.mask_wide, draws=dev, draw_w=_DRAW_W, hw=plan["hw"], flip=plan["flip"],
                                              trans_inv=plan["trans_inv"], line_depth=lab["line_depth"])
        return _batch(img, lab, [self.ids[p] for p in indices], [self.wh[p] for p in indices], draws, self.mean_size, plan["mixed"],
                      compact and (lambda counts: compact_labels(lab, counts, [d["crop"] for d in draws], cam_dis)), depth_map)


def save_results(results, output_dir="./outputs", class_name=("Car", "Pedestrian", "Cyclist")):
    """`KITTIDataset.save_results` (kitti.py:452-464) to the byte: {im_file: rows [cls, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry,
    score]} -> output_dir/preds/<im_file>, one line per row: the class name, '0.0 0', then every further value as ' {:.2f}'.
    -> the directory written (what `kitti_eval.eval_from_scratch` takes as det_dir)"""
    import os
    output_dir = os.path.join(output_dir, "preds")
    os.makedirs(output_dir, exist_ok=True)
    for img_file, rows in results.items():
        with open(os.path.join(output_dir, img_file), "w") as f:
            for row in rows:
                f.write("{} 0.0 0".format(class_name[int(row[0])]))
                for v in row[1:]:
                    f.write(" {:.2f}".format(v))
                f.write("\n")
    return output_dir


def build_test_batch(root_or_split_file, indices, device, img_mode="uint8", resolution=RESOLUTION):
    """`collate_fn([dataset[i] for i in indices])` of the reference's KITTIDataset for the unlabelled `testing/` split (kitti.py:116-135,
    :186-206, :395-431 with split == 'test': no augmentation, no labels): PNGs and calibrations are read on the host, the images resized
    by augment_images.  root_or_split_file: a split file (ImageSets/test.txt) or the KITTI root.  -> `img`, `calib` (B, 6) float64 (the
    six constants x ratio, :405-407), `info`, `im_file`, `ori_shape`, `ratio_pad` (B, 2, 2) float64 as build_batch(mode="val") gives
    them, and `P2` (B, 3, 4) float32, the projection of the original image (what the predictor's decode and corners need)."""
    import os
    import numpy as np
    from PIL import Image
    if torch.device(device).type != "cuda":
        raise Y3DError("build_test_batch: the batch is built on a HIP device (no host fallback)")
    if not len(indices):
        raise Y3DError("build_test_batch: no frames")
    data, ids = _split(root_or_split_file, "test")
    path = lambda sub, i, ext: os.path.join(data, sub, f"{i:06d}.{ext}")
    res = np.array([int(resolution[0]), int(resolution[1])])
    imgs, P2s, info, ratio_pad, calib = [], [], [], [], []
    for pos in indices:
        im = Image.open(path("image_2", ids[pos], "png"))
        img_size = np.array(im.size)
        P = read_calib(path("calib", ids[pos], "txt"))
        trans_inv = get_affine_transform(img_size / 2, img_size, resolution, inv=True)[1]
        rp = np.array([res / img_size, np.array([0, 0])])
        c = calib_params(P)
        calib.append([c[0] * rp[0, 0], c[1] * rp[0, 1], c[2] * rp[0, 0], c[3] * rp[0, 1], c[4] * rp[0, 0], c[5] * rp[0, 1]])
        imgs.append(torch.from_numpy(np.array(im.convert("RGB"))).to(device))
        P2s.append(P)
        ratio_pad.append(rp)
        info.append({"img_id": ids[pos], "img_size": img_size, "trans_inv": trans_inv})
    B = len(imgs)
    img = augment_images(imgs, [None] * B, [False] * B, [d["trans_inv"] for d in info], resolution, mode="float" if img_mode == "float" else "uint8")
    return {"img": img, "calib": upload(np.array(calib, np.float64), device, torch.float64), "info": info,
            "im_file": [f"{d['img_id']:06d}.txt" for d in info], "ori_shape": [d["img_size"][::-1] for d in info],
            "ratio_pad": upload(np.stack(ratio_pad).astype(np.float64), device, torch.float64), "P2": upload(np.stack(P2s), device, torch.float32)}
