"""KITTI 3D / BEV / 2D AP on the device — the evaluator behind `KITTIDataset.get_stats` (data/datasets/kitti.py:444-450).

Drop-ins for the reference's `data/datasets/kitti_eval.py`: `box_overlaps` (calculate_iou_partly :698-781), `eval_class`
(eval_class_v3 :815-947), `get_official_eval_result` (:1075-1165) and `eval_from_scratch` / `eval_from_scrach` (:1268-1336).  The
reference runs its rotated IoU as a numba.cuda kernel (NVIDIA only) and its matching as numba host loops; here the overlaps and both
passes of `compute_statistics_jit` are HIP kernels (csrc/kitti_eval.hip) and the tensors stay on the device between launches.  The host
parses text, scans the sorted true-positive scores for the 41 recall thresholds (`get_thresholds` :347-366) and turns the (41, 4)
count tables into AP.

One deliberate divergence: the reference splits the images into 50 parts and fails with fewer than 50 images; this has no parts.
"""
from __future__ import annotations

import io
import os

import numpy as np
import torch

from . import ops
from ._lib import Y3DError, lib

N_SAMPLE_PTS = 41
# clean_data's CLASS_NAMES (:370-373) -> the kernels' name codes (y3d.h)
_CLASS_NAMES = ("car", "pedestrian", "cyclist", "van", "person_sitting", "car", "tractor", "trailer")
_CODES = {n: i for i, n in enumerate(("car", "pedestrian", "cyclist", "van", "person_sitting", "tractor", "trailer"))}
CLASS_TO_NAME = {0: "Car", 1: "Pedestrian", 2: "Cyclist", 3: "Van", 4: "Person_sitting", 5: "car", 6: "tractor", 7: "trailer"}
_NAME_TO_CLASS = {v: n for n, v in CLASS_TO_NAME.items()}


def _name_codes(names):
    return np.array([_CODES.get(str(n).lower(), 7) + (8 if str(n) == "DontCare" else 0) for n in names], dtype=np.int32)


def _device(device):
    dev = torch.device(device if device is not None else "cuda")
    if dev.type != "cuda":
        raise Y3DError(f"kitti_eval runs on a HIP device, not {dev}")
    return dev


class Packed:
    """gt / dt annos of all images as the kernels take them (y3d.h): (N, 16) fp32 box records, int32 name codes, prefix offsets."""

    def __init__(self, gt_annos, dt_annos, device=None):
        if len(gt_annos) != len(dt_annos):
            raise Y3DError(f"kitti_eval: {len(gt_annos)} gt annos but {len(dt_annos)} det annos")
        if len(gt_annos) == 0:
            raise Y3DError("kitti_eval: no images")
        dev = _device(device)
        cap = lib().kitti_eval_max_boxes()
        self.n_img = len(gt_annos)
        ng = np.array([len(a["name"]) for a in gt_annos], dtype=np.int64)
        nd = np.array([len(a["name"]) for a in dt_annos], dtype=np.int64)
        if ng.max() > cap or nd.max() > cap:
            raise Y3DError(f"kitti_eval: an image has {int(ng.max())} gts / {int(nd.max())} dets; at most {cap} of each are supported")
        self.ng, self.nd = ng, nd
        self.total_gt = int(ng.sum())
        gt, gc = self._side(gt_annos, False)
        dt, dc = self._side(dt_annos, True)
        off = lambda n: np.concatenate(([0], np.cumsum(n)))
        self.gt_off_np = off(ng)
        self.dt_off_np = off(nd)
        self.ov_off_np = off(ng * nd)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.gt, self.gt_code, self.dt, self.dt_code = up(gt), up(gc), up(dt), up(dc)
        self.gt_off, self.dt_off = up(self.gt_off_np.astype(np.int32)), up(self.dt_off_np.astype(np.int32))
        self.ov_off = up(self.ov_off_np.astype(np.int64))
        self.device = dev
        self._ov = {}

    @staticmethod
    def _side(annos, det):
        counts = [len(a["name"]) for a in annos]
        n = sum(counts)
        rec = np.zeros((max(n, 1), 16), dtype=np.float32)
        codes = np.zeros(max(n, 1), dtype=np.int32)
        if n == 0:
            return rec, codes

        def field(k, width, default=None):
            parts = [np.asarray(a[k], dtype=np.float32).reshape(c, width) if (default is None or k in a) else np.full((c, width), default, np.float32)
                     for a, c in zip(annos, counts)]
            return np.concatenate(parts, 0)

        rec[:n, 0:4] = field("bbox", 4)
        rec[:n, 4:7] = field("location", 3)
        rec[:n, 7:10] = field("dimensions", 3)   # (l, h, w)
        rec[:n, 10:11] = field("rotation_y", 1)
        rec[:n, 11:12] = field("alpha", 1, -10.0)
        if det:
            rec[:n, 12:13] = field("score", 1)
        rec[:n, 13:14] = field("occluded", 1, 0.0)
        rec[:n, 14:15] = field("truncated", 1, 0.0)
        names, inv = np.unique(np.concatenate([np.asarray(a["name"]).reshape(-1) for a in annos]), return_inverse=True)
        codes[:n] = _name_codes(names)[inv.reshape(-1)]
        return rec, codes

    def overlaps(self, metric):
        """flat fp32 device tensor: image i's (n_dt, n_gt) block at ov_off[i]"""
        if metric not in (0, 1, 2):
            raise Y3DError(f"kitti_eval: unknown metric {metric}")
        if metric not in self._ov:
            ov = torch.zeros(max(int(self.ov_off_np[-1]), 1), dtype=torch.float32, device=self.device)
            lib().kitti_box_overlaps(metric, self.gt.data_ptr(), self.dt.data_ptr(), self.gt_off.data_ptr(), self.dt_off.data_ptr(),
                                     self.ov_off.data_ptr(), self.n_img, ov.data_ptr(), ops.stream())
            self._ov[metric] = ov
        return self._ov[metric]


def box_overlaps(gt_annos, dt_annos, metric, device=None):
    """The per-image blocks of calculate_iou_partly(dt_annos, gt_annos, metric): a list of (n_dt, n_gt) fp32 device tensors."""
    P = Packed(gt_annos, dt_annos, device)
    ov = P.overlaps(metric)
    o = P.ov_off_np
    return [ov[o[i]:o[i + 1]].view(int(P.nd[i]), int(P.ng[i])) for i in range(P.n_img)]


def get_thresholds(scores_desc, num_gt, num_sample_pts=N_SAMPLE_PTS):
    """get_thresholds (:347-366) on scores sorted in descending order.  Its skip test `(r - cur) < (cur - l)` only turns false as i grows,
    so each of the <= 41 recall steps is one vectorised search instead of a python pass over every true positive."""
    s = np.asarray(scores_desc, dtype=np.float64)
    n = s.shape[0]
    out = []
    if n == 0:
        return out
    i = np.arange(n)
    l_rec = (i + 1) / num_gt
    r_rec = np.where(i < n - 1, (i + 2) / num_gt, l_rec)
    last = i == n - 1
    cur, start = 0, 0
    while start < n:
        keep = ~((r_rec[start:] - cur) < (cur - l_rec[start:])) | last[start:]
        nz = np.flatnonzero(keep)
        if nz.size == 0:
            break
        idx = start + int(nz[0])
        out.append(s[idx])
        cur += 1 / (num_sample_pts - 1.0)
        start = idx + 1
    return out


def _eval_class(P, current_classes, difficultys, metric, min_overlaps, compute_aos):
    lb = lib()
    min_overlaps = np.asarray(min_overlaps, dtype=np.float64)
    nk, ncls, ndiff = min_overlaps.shape[0], len(current_classes), len(difficultys)
    if N_SAMPLE_PTS * nk > 256:
        raise Y3DError(f"kitti_eval: {nk} min-overlaps; at most {256 // N_SAMPLE_PTS} are supported")
    cd = np.array([[_CODES[_CLASS_NAMES[c]], d] for c in current_classes for d in difficultys], dtype=np.int32).reshape(-1, 2)
    if ndiff and (cd[:, 1].min() < 0 or cd[:, 1].max() > 2):
        raise Y3DError(f"kitti_eval: difficulties must be 0, 1 or 2, got {difficultys}")
    ncd, S = cd.shape[0], cd.shape[0] * nk
    mo = np.array([min_overlaps[k, metric, m] for m in range(ncls) for _ in range(ndiff) for k in range(nk)], dtype=np.float64)
    dev = P.device
    cd_d, mo_d = torch.from_numpy(cd).to(dev), torch.from_numpy(mo).to(dev)
    ov = P.overlaps(metric)
    tp = torch.full((S, max(P.total_gt, 1)), float("-inf"), dtype=torch.float32, device=dev)
    nvalid = torch.zeros(ncd, P.n_img, dtype=torch.int32, device=dev)
    args = (P.gt.data_ptr(), P.gt_code.data_ptr(), P.dt.data_ptr(), P.dt_code.data_ptr(), P.gt_off.data_ptr(), P.dt_off.data_ptr(),
            P.ov_off.data_ptr(), ov.data_ptr(), P.n_img)
    lb.kitti_eval_thresholds(*args, P.total_gt, metric, cd_d.data_ptr(), ncd, mo_d.data_ptr(), nk, tp.data_ptr(), nvalid.data_ptr(),
                             ops.stream())
    scores = torch.sort(tp, dim=1, descending=True)[0]
    ntp = (tp > float("-inf")).sum(1)
    head = torch.cat((ntp, nvalid.sum(1))).cpu().numpy()
    ntp, nvg = head[:S], head[S:]
    scores = scores[:, :max(int(ntp.max()), 1)].cpu().numpy()
    thr = np.zeros((S, N_SAMPLE_PTS), dtype=np.float32)
    nthr = np.zeros(S, dtype=np.int32)
    for s in range(S):
        t = get_thresholds(scores[s, :ntp[s]], nvg[s // nk])
        if len(t) > N_SAMPLE_PTS:
            raise Y3DError(f"kitti_eval: {len(t)} recall thresholds (the reference's table holds {N_SAMPLE_PTS})")
        thr[s, :len(t)] = t
        nthr[s] = len(t)
    thr_d, nthr_d = torch.from_numpy(thr).to(dev), torch.from_numpy(nthr).to(dev)
    cnt = torch.empty(S * N_SAMPLE_PTS * P.n_img * 3, dtype=torch.int32, device=dev)
    sim = torch.empty(S * N_SAMPLE_PTS * P.n_img, dtype=torch.float64, device=dev)
    pr = torch.empty(S, N_SAMPLE_PTS, 4, dtype=torch.float64, device=dev)
    lb.kitti_eval_counts(*args, metric, cd_d.data_ptr(), ncd, mo_d.data_ptr(), nk, thr_d.data_ptr(), nthr_d.data_ptr(), int(bool(compute_aos)),
                         cnt.data_ptr(), sim.data_ptr(), pr.data_ptr(), ops.stream())
    pr = pr.cpu().numpy()
    shape = (ncls, ndiff, nk, N_SAMPLE_PTS)
    precision, recall, aos, all_thr = np.zeros(shape), np.zeros(shape), np.zeros(shape), np.zeros(shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        for m in range(ncls):
            for l in range(ndiff):
                for k in range(nk):
                    s = (m * ndiff + l) * nk + k
                    n = nthr[s]
                    all_thr[m, l, k, :n] = thr[s, :n]
                    p = pr[s]
                    precision[m, l, k, :n] = p[:n, 0] / (p[:n, 0] + p[:n, 1])   # 0/0 = NaN, as numpy gives the reference
                    if compute_aos:
                        aos[m, l, k, :n] = p[:n, 3] / (p[:n, 0] + p[:n, 1])
                    for i in range(n):
                        precision[m, l, k, i] = np.max(precision[m, l, k, i:], axis=-1)
                        if compute_aos:
                            aos[m, l, k, i] = np.max(aos[m, l, k, i:], axis=-1)
    return {"recall": recall, "precision": precision, "orientation": aos, "thresholds": all_thr, "min_overlaps": min_overlaps}


def eval_class(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos=False, z_axis=1, z_center=1.0,
               num_parts=50, device=None):
    """eval_class_v3 (:815-947): {recall (all zero, as the reference leaves it), precision (suffix max applied), orientation,
    thresholds, min_overlaps}, each (num_class, num_difficulty, num_minoverlap, 41).  num_parts is accepted and ignored."""
    _check_axes(z_axis, z_center)
    return _eval_class(Packed(gt_annos, dt_annos, device), list(current_classes), list(difficultys), metric, min_overlaps, compute_aos)


def get_mAP(prec, ap_mode=40):
    """get_mAP (:950-961)"""
    sums = 0
    if ap_mode == 40:
        for i in range(1, prec.shape[-1], 1):
            sums = sums + prec[..., i]
        return sums / 40 * 100
    if ap_mode == 11:
        for i in range(0, prec.shape[-1], 4):
            sums = sums + prec[..., i]
        return sums / 11 * 100
    raise Y3DError(f"ap_mode must be 40 or 11, got {ap_mode}")


def _check_axes(z_axis, z_center):
    if z_axis != 1 or z_center != 1.0:
        raise Y3DError(f"kitti_eval: only the KITTI camera frame (z_axis = 1, z_center = 1.0) is supported, got {z_axis}, {z_center}")


def _print_str(value, *arg):
    s = io.StringIO()
    print(value, *arg, file=s)
    return s.getvalue()


def get_official_eval_result(gt_annos, dt_annos, current_classes, difficultys=(0, 1, 2), z_axis=1, z_center=1.0, ap_mode=40, device=None,
                             _packed=None):
    """get_official_eval_result (:1075-1165): {"result": str, "detail": {class name: {"bbox@0.70": [easy, moderate, hard], ...}}}"""
    _check_axes(z_axis, z_center)
    overlap_mod = np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.7, 0.7, 0.7],
                            [0.7, 0.5, 0.5, 0.7, 0.5, 0.7, 0.7, 0.7],
                            [0.7, 0.5, 0.5, 0.7, 0.5, 0.7, 0.7, 0.7]])
    overlap_easy = np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.5, 0.5, 0.5],
                             [0.5, 0.25, 0.25, 0.5, 0.25, 0.5, 0.5, 0.5],
                             [0.5, 0.25, 0.25, 0.5, 0.25, 0.5, 0.5, 0.5]])
    overlap_easy2 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.5, 0.5, 0.5],
                              [0.3, 0.25, 0.25, 0.5, 0.25, 0.5, 0.5, 0.5],
                              [0.3, 0.25, 0.25, 0.5, 0.25, 0.5, 0.5, 0.5]])
    min_overlaps = np.stack([overlap_mod, overlap_easy, overlap_easy2], axis=0)
    if not isinstance(current_classes, (list, tuple)):
        current_classes = [current_classes]
    current_classes = [_NAME_TO_CLASS[c] if isinstance(c, str) else int(c) for c in current_classes]
    for c in current_classes:
        if c not in CLASS_TO_NAME:
            raise Y3DError(f"kitti_eval: unknown class {c}")
    min_overlaps = min_overlaps[:, :, current_classes]
    compute_aos = False
    for anno in dt_annos:
        if np.asarray(anno["alpha"]).shape[0] != 0:
            if np.asarray(anno["alpha"])[0] != -10:
                compute_aos = True
            break
    P = _packed if _packed is not None else Packed(gt_annos, dt_annos, device)
    difficultys = list(difficultys)
    metrics = {t: _eval_class(P, current_classes, difficultys, i, min_overlaps, compute_aos) for i, t in enumerate(("bbox", "bev", "3d"))}
    result, detail = "", {}
    for j, curcls in enumerate(current_classes):
        class_name = CLASS_TO_NAME[curcls]
        detail[class_name] = {}
        for i in range(min_overlaps.shape[0]):
            mAPbbox = get_mAP(metrics["bbox"]["precision"][j, :, i], ap_mode)
            mAPbev = get_mAP(metrics["bev"]["precision"][j, :, i], ap_mode)
            mAP3d = get_mAP(metrics["3d"]["precision"][j, :, i], ap_mode)
            detail[class_name][f"bbox@{min_overlaps[i, 0, j]:.2f}"] = mAPbbox.tolist()
            detail[class_name][f"bev@{min_overlaps[i, 1, j]:.2f}"] = mAPbev.tolist()
            detail[class_name][f"3d@{min_overlaps[i, 2, j]:.2f}"] = mAP3d.tolist()
            result += _print_str(f"{class_name} AP(Average Precision)@{min_overlaps[i, 0, j]:.2f}, {min_overlaps[i, 1, j]:.2f}, "
                                 f"{min_overlaps[i, 2, j]:.2f}:")
            result += _print_str("bbox AP:" + ", ".join(f"{v:.2f}" for v in mAPbbox))
            result += _print_str("bev  AP:" + ", ".join(f"{v:.2f}" for v in mAPbev))
            result += _print_str("3d   AP:" + ", ".join(f"{v:.2f}" for v in mAP3d))
            if compute_aos:
                mAPaos = get_mAP(metrics["bbox"]["orientation"][j, :, i], ap_mode)
                detail[class_name]["aos"] = mAPaos.tolist()
                result += _print_str("aos  AP:" + ", ".join(f"{v:.2f}" for v in mAPaos))
    return {"result": result, "detail": detail}


# ------------------------------------------------------------------------------------------------------------------------------
# text files (eval_from_scrach :1268-1336) and the validator's entry (KITTIDataset.get_stats / save_results, kitti.py:444-464)
# ------------------------------------------------------------------------------------------------------------------------------
def _annos_from_table(t, det):
    """(N, 15 | 16) table of strings in KITTI label order -> the reference's anno dict (float32 fields, dimensions as (l, h, w))"""
    f = lambda cols: t[:, cols].astype(np.float32)
    a = {"bbox": f(slice(4, 8)), "alpha": f(3), "occluded": f(2), "truncated": f(1), "name": t[:, 0], "location": f(slice(11, 14)),
         "dimensions": f([10, 8, 9]), "rotation_y": f(14)}
    if det:
        a["score"] = f(15)
    return a


def read_label_file(path, det=False):
    """One KITTI label (15 columns) or detection (16 columns) file -> anno dict, as eval_from_scrach parses it (np.loadtxt(dtype=str))."""
    with open(path) as fh:
        toks = fh.read().split()
    return _annos_from_table(np.array(toks, dtype=str).reshape(-1, 16 if det else 15), det)


def _run_classes(all_gt, all_det, eval_cls_list, ap_mode, device, verbose):
    P = Packed(all_gt, all_det, device)
    res = None
    for cls in eval_cls_list:
        res = get_official_eval_result(all_gt, all_det, cls, ap_mode=ap_mode, _packed=P)["detail"][cls]
        if verbose:
            print("*" * 20 + cls + "*" * 20)
            for k in res.keys():
                print(k, res[k])
    return res


def eval_from_scratch(gt_dir, det_dir, eval_cls_list=None, ap_mode=40, device=None, verbose=False):
    """eval_from_scrach (:1268-1336): every file of det_dir against the same-named label file of gt_dir; returns the detail dict of
    the last class of eval_cls_list (default Cyclist, Pedestrian, Car), AP40 or AP11."""
    if eval_cls_list is None:
        eval_cls_list = ["Cyclist", "Pedestrian", "Car"]
    files = sorted(os.listdir(det_dir))
    all_gt = [read_label_file(os.path.join(gt_dir, f)) for f in files]
    all_det = [read_label_file(os.path.join(det_dir, f), det=True) for f in files]
    return _run_classes(all_gt, all_det, eval_cls_list, ap_mode, device, verbose)


eval_from_scrach = eval_from_scratch


def results_to_annos(results, class_name=("Car", "Pedestrian", "Cyclist")):
    """{im_file: rows [cls, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, score]} (kitti.decode_preds_eval) -> (sorted im_files, det annos)
    with every value rounded as save_results writes and eval_from_scrach reads it: '{:.2f}' text, read back as float32."""
    files = sorted(results)
    annos = []
    for f in files:
        r = np.asarray(results[f], dtype=np.float64).reshape(-1, 14)
        t = np.empty((r.shape[0], 16), dtype=object)
        t[:, 0] = [class_name[int(c)] for c in r[:, 0]]
        t[:, 1], t[:, 2] = "0.0", "0"
        t[:, 3:] = np.char.mod("%.2f", r[:, 1:]) if r.shape[0] else np.zeros((0, 13), dtype=str)
        annos.append(_annos_from_table(t.astype(str), True))
    return files, annos


def get_stats(results, label_dir, class_name=("Car", "Pedestrian", "Cyclist"), eval_cls_list=None, ap_mode=40, device=None):
    """KITTIDataset.get_stats (kitti.py:444-450) without files: the Car moderate 3D AP at IoU 0.7 (AP40 by default) of the decoded
    detections against label_dir, equal to what the reference computes from the files save_results would write."""
    if eval_cls_list is None:
        eval_cls_list = ["Cyclist", "Pedestrian", "Car"]
    files, dets = results_to_annos(results, class_name)
    gts = [read_label_file(os.path.join(label_dir, f)) for f in files]
    return _run_classes(gts, dets, eval_cls_list, ap_mode, device, False)["3d@0.70"][1]
