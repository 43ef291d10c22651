"""Axis-aligned 3D box detection AP: the reference's tools/eval_det.py (VoteNet's eval_det) with the
same signatures, return values and dict key order, plus a keyword-only ``device`` (None: the GPU when
one is available), and ``evaluate_box_ap``, the script's ``__main__`` on the per-scan lists that
tools/test.py collects.

Every detection's best GT -- (ovmax, jmax), the first GT of its (class, image) with the strictly
largest ``get_iou`` -- depends neither on the order of the detections nor on the threshold; the
reference's greedy pass only decides which detection gets a GT that several point at: the earliest
in confidence order among those with ovmax > ovthresh.  On the GPU ``sg_det_match`` computes
(ovmax, jmax) for every class at once and resolves the claims for all thresholds in the same launch
pair; boxes come from ``sg_det_boxes_runs`` / ``sg_det_boxes_labels``.  The O(detections) rest stays
here, copied from the reference: ``np.argsort(-confidence)`` (numpy's default kind, whose tie order
the device path takes as given), the cumulative sums, rec / prec and ``voc_ap``.

Without a GPU (or with a user-supplied ``get_iou_func``) a numpy restatement of the reference loop
runs instead: the same IoU operations, vectorised over each detection's GT boxes, and the same
greedy pass.  Quirks are kept: ``eval_det`` raises KeyError for a GT class without predictions, where
``eval_sphere`` reports 0; a class with predictions and no GT has npos = 0 and numpy's nan / inf
recall.

Yaw-oriented boxes (no counterpart in the reference): ``get_iou_obb`` / ``get_iou_bev`` score 7-number
boxes (cx, cy, cz, du, dv, dz, theta) by the rules of ``softgroup_amd.ops.boxes``; passed as
``get_iou_func`` they take ``sg_det_match_obb`` on the GPU and a vectorised numpy path without one, both
equal to the reference loop with the same function.  ``oriented_instance_boxes`` forms such boxes
through ``describe_instances``, and ``evaluate_box_ap(boxes='obb')`` scores them; with the default
``boxes='aabb'`` nothing changes.
"""
import numpy as np

from .instance_eval import _runs_of
from .point_wise_eval import host, use_device

MAX_THRESHOLDS = 16          # SG_DET_MAX_THRESHOLDS
_BAD_COORD = 1               # SG_DET_BAD_COORD


# ------------------------------------------------------------------ the reference's functions
def voc_ap(rec, prec, use_07_metric=False):
    """ap = voc_ap(rec, prec, [use_07_metric]): VOC AP from precision and recall; the VOC07
    11-point method when use_07_metric is true."""
    if use_07_metric:
        ap = 0.
        for t in np.arange(0., 1.1, 0.1):
            if np.sum(rec >= t) == 0:
                p = 0
            else:
                p = np.max(prec[rec >= t])
            ap = ap + p / 11.
    else:
        mrec = np.concatenate(([0.], rec, [1.]))
        mpre = np.concatenate(([0.], prec, [0.]))
        for i in range(mpre.size - 1, 0, -1):             # precision envelope
            mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
        i = np.where(mrec[1:] != mrec[:-1])[0]             # where recall changes
        ap = np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])
    return ap


def get_iou(box_a, box_b, eps=1e-10):
    """IoU of two axis-aligned boxes given as (xmin ymin zmin xmax ymax zmax)."""
    min_max = np.array([box_a[3:], box_b[3:]]).min(0)
    max_min = np.array([box_a[0:3], box_b[0:3]]).max(0)
    if not ((min_max > max_min).all()):
        return 0.0
    intersection = (min_max - max_min).prod()
    vol_a = (box_a[3:6] - box_a[:3]).prod()
    vol_b = (box_b[3:6] - box_b[:3]).prod()
    union = vol_a + vol_b - intersection
    return 1.0 * intersection / union


def get_iou_obb(box_a, box_b):
    """IoU of two yaw-oriented boxes given as (cx cy cz du dv dz theta): the definition of
    ``softgroup_amd.ops.boxes``.  Usable as the ``get_iou_func`` of eval_det_cls / eval_det /
    eval_sphere, which then match on the device (or vectorised) when every box has 7 numbers."""
    from ..ops import boxes as BX
    return BX.obb_iou_pair(BX.boxes8(box_a)[0], BX.boxes8(box_b)[0], '3d')


def get_iou_bev(box_a, box_b):
    """get_iou_obb in the bird's-eye view: the IoU of the two rectangles in the xy plane."""
    from ..ops import boxes as BX
    return BX.obb_iou_pair(BX.boxes8(box_a)[0], BX.boxes8(box_b)[0], 'bev')


def _iou_rows(bb, gts):
    """get_iou(bb, g) for every row g of gts [k, 6] (fp64), operation for operation"""
    min_max = np.minimum(bb[3:], gts[:, 3:])
    max_min = np.maximum(bb[:3], gts[:, :3])
    ok = (min_max > max_min).all(1)
    d = min_max - max_min
    inter = (d[:, 0] * d[:, 1]) * d[:, 2]
    wa = bb[3:6] - bb[:3]
    vol_a = (wa[0] * wa[1]) * wa[2]
    wb = gts[:, 3:6] - gts[:, :3]
    vol_b = (wb[:, 0] * wb[:, 1]) * wb[:, 2]
    with np.errstate(all='ignore'):
        iou = inter / ((vol_a + vol_b) - inter)
    return np.where(ok, iou, 0.0)


class _ClassJob:
    """eval_det_cls's tables for one class: class_recs (GT per image, in the reference's order) and
    the detections in insertion order with the sorted order."""

    def __init__(self, pred, gt):
        self.gt_sphere = {}
        self.npos = 0
        for img_id in gt.keys():
            sphere = np.array(gt[img_id])
            self.npos += len(sphere)
            self.gt_sphere[img_id] = sphere
        for img_id in pred.keys():
            if img_id not in gt:
                self.gt_sphere[img_id] = np.array([])
        self.image_ids, confidence, BB = [], [], []
        for img_id in pred.keys():
            for sphere, score in pred[img_id]:
                self.image_ids.append(img_id)
                confidence.append(score)
                BB.append(sphere)
        self.confidence = np.array(confidence)
        self.BB = np.array(BB)
        self.sorted_ind = np.argsort(-self.confidence)
        self.nd = len(self.image_ids)

    def boxes6(self):
        """the detection and GT boxes as fp64 [k, 6] arrays, or None when the default get_iou cannot
        be restated on them (not six numbers per box)"""
        if self.nd and (self.BB.ndim != 2 or self.BB.shape[1] != 6):
            return None
        for s in self.gt_sphere.values():
            if s.size and (s.ndim != 2 or s.shape[1] != 6):
                return None
        return True

    def boxes7(self):
        """True when every detection and GT box has seven numbers (the oriented IoU's fast paths)"""
        if self.nd and (self.BB.ndim != 2 or self.BB.shape[1] != 7):
            return None
        for s in self.gt_sphere.values():
            if s.size and (s.ndim != 2 or s.shape[1] != 7):
                return None
        return True

    def finish(self, tp_flags, use_07_metric):
        """rec, prec, ap from the TP flags in sorted order (eval_det.py:147-158)"""
        tp = np.asarray(tp_flags, dtype=np.float64)
        fp = 1.0 - tp
        fp = np.cumsum(fp)
        tp = np.cumsum(tp)
        rec = tp / float(self.npos)
        prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
        ap = voc_ap(rec, prec, use_07_metric)
        return rec, prec, ap


def _greedy(ov, jm, img_of, ovthresh):
    """the reference's TP pass over detections in sorted order, given (ovmax, jmax) per detection"""
    tp = np.zeros(len(ov), np.uint8)
    taken = set()
    for d in range(len(ov)):
        if ov[d] > ovthresh:
            key = (img_of[d], jm[d])
            if key not in taken:
                tp[d] = 1
                taken.add(key)
    return tp


def _match_reference_loop(job, ovthreshs, get_iou_func):
    """eval_det_cls's loop as written (any box shape, any IoU function) -> TP flags per threshold in
    sorted order"""
    BB = job.BB[job.sorted_ind, ...]
    image_ids = [job.image_ids[x] for x in job.sorted_ind]
    ov = np.full(job.nd, -np.inf)
    jm = np.full(job.nd, -1, np.int64)
    for d in range(job.nd):
        bb = BB[d, ...].astype(float)
        BBGT = job.gt_sphere[image_ids[d]].astype(float)
        ovmax = -np.inf
        if BBGT.size > 0:
            for j in range(BBGT.shape[0]):
                iou = get_iou_func(bb, BBGT[j, ...])
                if iou > ovmax:
                    ovmax = iou
                    jm[d] = j
        ov[d] = ovmax
    return [_greedy(ov, jm, image_ids, t) for t in ovthreshs]


def _match_numpy(job, ovthreshs):
    """(ovmax, jmax) vectorised per image with the default get_iou, then the greedy pass"""
    img_of = [job.image_ids[x] for x in job.sorted_ind]
    BB = job.BB[job.sorted_ind, ...].astype(float) if job.nd else np.zeros((0, 6))
    ov = np.full(job.nd, -np.inf)
    jm = np.full(job.nd, -1, np.int64)
    for d in range(job.nd):
        G = job.gt_sphere[img_of[d]].astype(float)
        if G.size == 0:
            continue
        iou = _iou_rows(BB[d], G)
        cand = np.where(np.isnan(iou), -np.inf, iou)       # NaN never wins `iou > ovmax`
        j = int(np.argmax(cand))
        if cand[j] > -np.inf:
            ov[d], jm[d] = cand[j], j
    return [_greedy(ov, jm, img_of, t) for t in ovthreshs]


def _match_numpy_obb(job, ovthreshs, mode):
    """(ovmax, jmax) with the oriented IoU, one vectorised IoU matrix per image, then the greedy pass"""
    from ..ops import boxes as BX
    img_of = [job.image_ids[x] for x in job.sorted_ind]
    BB = BX.boxes8(job.BB[job.sorted_ind, ...].astype(float)) if job.nd else np.zeros((0, 8))
    ov = np.full(job.nd, -np.inf)
    jm = np.full(job.nd, -1, np.int64)
    rows_of = {}
    for d, img_id in enumerate(img_of):
        rows_of.setdefault(img_id, []).append(d)
    for img_id, rows in rows_of.items():
        G = job.gt_sphere[img_id].astype(float)
        if G.size == 0:
            continue
        rows = np.asarray(rows)
        iou = BX.box_iou_numpy(BB[rows], BX.boxes8(G), mode)
        cand = np.where(np.isnan(iou), -np.inf, iou)       # NaN never wins `iou > ovmax`
        j = np.argmax(cand, axis=1)                        # the first of the largest
        best = cand[np.arange(len(rows)), j]
        hit = best > -np.inf
        ov[rows[hit]], jm[rows[hit]] = best[hit], j[hit]
    return [_greedy(ov, jm, img_of, t) for t in ovthreshs]


def _match_device(jobs, ovthreshs, device, mode=None):
    """TP flags per (job, threshold) in each job's sorted order, for all jobs in one sg_det_match
    (mode None: six-number boxes) or one sg_det_match_obb (mode '3d' / 'bev': seven-number boxes)"""
    import torch
    if mode is None:
        width, rows = 6, (lambda b: np.asarray(b, np.float64).reshape(-1, 6))
    else:
        from ..ops import boxes as BX
        width, rows = 8, (lambda b: BX.boxes8(np.asarray(b, np.float64).reshape(-1, 7)))
    dev = torch.device('cuda' if device is None else device)
    det_box, det_group, det_rank, gt_box, group_sizes = [], [], [], [], []
    for job in jobs:
        groups = {img_id: len(group_sizes) + k for k, img_id in enumerate(job.gt_sphere)}
        for img_id, s in job.gt_sphere.items():
            group_sizes.append(len(s) if s.size else 0)
            if s.size:
                gt_box.append(rows(s))
        if job.nd:
            det_box.append(rows(job.BB))
            det_group.append(np.array([groups[i] for i in job.image_ids], np.int32))
            rank = np.empty(job.nd, np.int32)
            rank[job.sorted_ind] = np.arange(job.nd, dtype=np.int32)
            det_rank.append(rank)
    n_det = sum(j.nd for j in jobs)
    if n_det == 0:
        return [[np.zeros(0, np.uint8) for _ in ovthreshs] for _ in jobs]
    tp = match_boxes(np.concatenate(det_box), np.concatenate(det_group), np.concatenate(det_rank),
                     np.concatenate(gt_box) if gt_box else np.zeros((0, width)), np.asarray(group_sizes, np.int64),
                     ovthreshs, dev, mode)[2]
    out, o = [], 0
    for job in jobs:
        out.append([tp[k, o:o + job.nd][job.sorted_ind] for k in range(len(ovthreshs))])
        o += job.nd
    return out


def match_boxes(det_box, det_group, det_rank, gt_box, group_sizes, ovthreshs, device, mode=None):
    """sg_det_match on host arrays -> (ovmax [n_det] fp64, jmax [n_det] global GT row, tp
    [n_thr, n_det] uint8), numpy arrays.  With mode '3d' / 'bev' the boxes are box rows of 8 doubles
    (``softgroup_amd.ops.boxes.boxes8``) and sg_det_match_obb runs; an invalid box raises ValueError."""
    import torch
    width = 6
    if mode is not None:
        from ..ops import boxes as BX
        BX._mode(mode)
        width = 8
        BX._check(BX._rows8(det_box, 'det_box'), 'match_boxes')
        BX._check(BX._rows8(np.asarray(gt_box, np.float64).reshape(-1, 8), 'gt_box'), 'match_boxes')
    ovthreshs = [float(t) for t in ovthreshs]
    assert 1 <= len(ovthreshs) <= MAX_THRESHOLDS
    n_det, n_gt = len(det_group), len(gt_box)
    off = np.concatenate([[0], np.cumsum(group_sizes)]).astype(np.int64)
    d_det = torch.from_numpy(np.ascontiguousarray(det_box, np.float64)).to(device)
    d_grp = torch.from_numpy(np.ascontiguousarray(det_group, np.int32)).to(device)
    d_rank = torch.from_numpy(np.ascontiguousarray(det_rank, np.int32)).to(device)
    d_gt = torch.from_numpy(np.ascontiguousarray(gt_box, np.float64).reshape(-1, width)).to(device)
    d_off = torch.from_numpy(off).to(device)
    return _match_launch(d_det, d_grp, d_rank, n_det, d_gt, d_off, n_gt, ovthreshs, mode)


def _match_launch(d_det, d_grp, d_rank, n_det, d_gt, d_off, n_gt, ovthreshs, mode=None):
    import ctypes
    import torch
    from .. import _lib as L
    dev = d_det.device
    th = (ctypes.c_double * len(ovthreshs))(*ovthreshs)
    ovmax = torch.empty(n_det, dtype=torch.float64, device=dev)
    jmax = torch.empty(n_det, dtype=torch.int64, device=dev)
    tp = torch.empty((len(ovthreshs), n_det), dtype=torch.uint8, device=dev)
    if mode is not None:
        from ..ops import boxes as BX
        ws = L.workspace(L.lib().sg_det_match_obb_workspace_bytes(n_gt, len(ovthreshs)), dev)
        L.check(L.lib().sg_det_match_obb(L.ptr(d_det), L.ptr(d_grp), L.ptr(d_rank), n_det, L.ptr(d_gt), L.ptr(d_off),
                                         n_gt, ctypes.cast(th, ctypes.c_void_p), len(ovthreshs), BX._mode(mode),
                                         L.ptr(ovmax), L.ptr(jmax), L.ptr(tp), L.ptr(ws), ws.numel(), L.stream()),
                'sg_det_match_obb')
        return ovmax.cpu().numpy(), jmax.cpu().numpy(), tp.cpu().numpy()
    ws = L.workspace(L.lib().sg_det_match_workspace_bytes(n_gt, len(ovthreshs)), dev)
    L.check(L.lib().sg_det_match(L.ptr(d_det), L.ptr(d_grp), L.ptr(d_rank), n_det, L.ptr(d_gt), L.ptr(d_off), n_gt,
                                 ctypes.cast(th, ctypes.c_void_p), len(ovthreshs), L.ptr(ovmax), L.ptr(jmax),
                                 L.ptr(tp), L.ptr(ws), ws.numel(), L.stream()), 'sg_det_match')
    return ovmax.cpu().numpy(), jmax.cpu().numpy(), tp.cpu().numpy()


def _eval_jobs(jobs, ovthreshs, use_07_metric, get_iou_func, device):
    """[(rec, prec, ap) per threshold] per job"""
    obb = '3d' if get_iou_func is get_iou_obb else 'bev' if get_iou_func is get_iou_bev else None
    if obb is not None and all(job.boxes7() for job in jobs):
        if use_device(device) and len(ovthreshs) <= MAX_THRESHOLDS:
            flags = _match_device(jobs, ovthreshs, device, obb)
        else:
            flags = [_match_numpy_obb(job, ovthreshs, obb) for job in jobs]
    elif get_iou_func is not get_iou or any(job.boxes6() is None for job in jobs):
        flags = [_match_reference_loop(job, ovthreshs, get_iou_func) for job in jobs]
    elif use_device(device) and len(ovthreshs) <= MAX_THRESHOLDS:
        flags = _match_device(jobs, ovthreshs, device)
    else:
        flags = [_match_numpy(job, ovthreshs) for job in jobs]
    return [[job.finish(f, use_07_metric) for f in fl] for job, fl in zip(jobs, flags)]


def eval_det_cls(pred, gt, ovthresh=0.25, use_07_metric=False, get_iou_func=get_iou, *, device=None):
    """Precision / recall / AP of one class.
    pred: {img_id: [(box, score)]}, gt: {img_id: [box]} -> (rec [nd], prec [nd], ap)"""
    return _eval_jobs([_ClassJob(pred, gt)], [ovthresh], use_07_metric, get_iou_func, device)[0][0]


def _by_class(pred_all, gt_all):
    """eval_det's regrouping: ({classname: {img_id: [(box, score)]}}, {classname: {img_id: [box]}})"""
    pred, gt = {}, {}
    for img_id in pred_all.keys():
        for classname, sphere, score in pred_all[img_id]:
            if classname not in pred:
                pred[classname] = {}
            if img_id not in pred[classname]:
                pred[classname][img_id] = []
            if classname not in gt:
                gt[classname] = {}
            if img_id not in gt[classname]:
                gt[classname][img_id] = []
            pred[classname][img_id].append((sphere, score))
    for img_id in gt_all.keys():
        for classname, sphere in gt_all[img_id]:
            if classname not in gt:
                gt[classname] = {}
            if img_id not in gt[classname]:
                gt[classname][img_id] = []
            gt[classname][img_id].append(sphere)
    return pred, gt


def _eval_multi(pred_all, gt_all, ovthreshs, use_07_metric, get_iou_func, device, missing):
    """eval_det (missing='raise') / eval_sphere (missing='zero') for several thresholds at once ->
    [(rec, prec, ap) dicts] per threshold"""
    pred, gt = _by_class(pred_all, gt_all)
    if missing == 'raise':
        for classname in gt.keys():
            if classname not in pred:
                raise KeyError(classname)
    names = [c for c in gt.keys() if c in pred]
    res = _eval_jobs([_ClassJob(pred[c], gt[c]) for c in names], ovthreshs, use_07_metric, get_iou_func, device)
    res = dict(zip(names, res))
    out = []
    for k in range(len(ovthreshs)):
        rec, prec, ap = {}, {}, {}
        for classname in gt.keys():
            if classname in res:
                rec[classname], prec[classname], ap[classname] = res[classname][k]
            else:
                rec[classname] = 0
                prec[classname] = 0
                ap[classname] = 0
        out.append((rec, prec, ap))
    return out


def eval_det(pred_all, gt_all, ovthresh=0.25, use_07_metric=False, get_iou_func=get_iou, *, device=None):
    """Precision / recall / AP per class.
    pred_all: {img_id: [(classname, box, score)]}, gt_all: {img_id: [(classname, box)]}
    -> ({classname: rec}, {classname: prec}, {classname: ap}); KeyError for a GT class without
    predictions."""
    return _eval_multi(pred_all, gt_all, [ovthresh], use_07_metric, get_iou_func, device, 'raise')[0]


def eval_sphere(pred_all, gt_all, ovthresh=0.25, use_07_metric=False, get_iou_func=get_iou, *, device=None):
    """eval_det, where a GT class without predictions gets rec = prec = ap = 0."""
    return _eval_multi(pred_all, gt_all, [ovthresh], use_07_metric, get_iou_func, device, 'zero')[0]


# ------------------------------------------------------------------ boxes of masks and instances
def _coords_dtype(coords):
    names = {str(getattr(c, 'dtype', None)).replace('torch.', '') for c in coords}
    return 'float32' if names <= {'float32'} else 'float64'


def _boxes_numpy(coords, runs, labels):
    """pred boxes per scan from runs, and GT (boxes, count, first) per scan from labels"""
    pred_boxes = []
    for c, scan_runs in zip(coords, runs):
        c = host(c)
        for s, n in scan_runs:
            off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
            idx = np.arange(int(n.sum())) + np.repeat(s - off, n)     # the mask's points, in order
            inst = c[idx]
            pred_boxes.append(np.concatenate([inst.min(0), inst.max(0)]).astype(np.float64))
    gt = []
    for c, lab in zip(coords, labels):
        c, lab = host(c), host(lab).astype(np.int64)
        k = int(lab.max()) + 1 if lab.size else 0
        valid = np.flatnonzero((lab >= 0) & (lab < k))
        order = valid[np.argsort(lab[valid], kind='stable')]
        count = np.bincount(lab[valid], minlength=max(k, 0))[:max(k, 0)]
        first = np.full(max(k, 0), -1, np.int64)
        boxes = np.full((max(k, 0), 6), np.nan)
        starts = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64) if k > 0 else np.zeros(0, np.int64)
        for i in np.flatnonzero(count):
            pts = order[starts[i]:starts[i] + count[i]]
            first[i] = pts[0]
            inst = c[pts]
            boxes[i] = np.concatenate([inst.min(0), inst.max(0)])
        gt.append((boxes, count.astype(np.int64), first))
    return pred_boxes, gt


def _boxes_device(coords, runs, labels, device):
    """the same on the GPU: one sg_det_boxes_runs for every mask of every scan and one
    sg_det_boxes_labels for every instance; None when a coordinate is not finite"""
    import torch
    from .. import _lib as L
    dev = torch.device('cuda' if device is None else device)
    tdt = torch.float32 if _coords_dtype(coords) == 'float32' else torch.float64
    sizes = [int(c.shape[0]) for c in coords]
    d_coords = torch.cat([(c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c)))
                          .to(device=dev, dtype=tdt).reshape(-1, 3) for c in coords]) if coords else \
        torch.zeros((0, 3), dtype=tdt, device=dev)
    scan_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    f64 = int(tdt == torch.float64)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)

    starts, lens, owner, n_pred = [], [], [], 0
    for si, scan_runs in enumerate(runs):
        for s, n in scan_runs:
            starts.append(s + scan_off[si])
            lens.append(n)
            owner.append(np.full(len(s), n_pred, np.int32))
            n_pred += 1
    cat = (lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt))  # noqa: E731
    starts, lens, owner = cat(starts, np.int64), cat(lens, np.int64), cat(owner, np.int32)
    run_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pboxes = torch.empty((n_pred, 6), dtype=torch.float64, device=dev)
    d_s, d_o, d_w = (torch.from_numpy(a).to(dev) for a in (starts, run_off, owner))
    L.check(L.lib().sg_det_boxes_runs(L.ptr(d_coords), f64, L.ptr(d_s), L.ptr(d_o), L.ptr(d_w), len(starts),
                                      int(run_off[-1]), n_pred, L.ptr(pboxes), L.ptr(flags), L.stream()),
            'sg_det_boxes_runs')

    d_lab = torch.cat([(lab if isinstance(lab, torch.Tensor) else torch.from_numpy(np.asarray(lab)))
                       .to(device=dev, dtype=torch.int64).reshape(-1) for lab in labels]) if labels else \
        torch.zeros(0, dtype=torch.int64, device=dev)
    n_inst = [int(x) + 1 for x in torch.stack([lab.max() if lab.numel() else torch.tensor(-1, device=dev)
                                               for lab in torch.split(d_lab, sizes)]).cpu().tolist()] \
        if sizes else []
    n_inst = [max(k, 0) for k in n_inst]
    owner_off = np.concatenate([[0], np.cumsum(n_inst)]).astype(np.int64)
    n_gt = int(owner_off[-1])
    gboxes = torch.empty((n_gt, 6), dtype=torch.float64, device=dev)
    count = torch.empty(n_gt, dtype=torch.int64, device=dev)
    first = torch.empty(n_gt, dtype=torch.int64, device=dev)
    d_so, d_oo = torch.from_numpy(scan_off).to(dev), torch.from_numpy(owner_off).to(dev)
    L.check(L.lib().sg_det_boxes_labels(L.ptr(d_coords), f64, L.ptr(d_lab), L.ptr(d_so), L.ptr(d_oo),
                                        max(len(sizes), 1), int(scan_off[-1]), n_gt, L.ptr(gboxes), L.ptr(count),
                                        L.ptr(first), L.ptr(flags), L.stream()), 'sg_det_boxes_labels')
    if int(flags.item()) & _BAD_COORD:
        return None
    pb = pboxes.cpu().numpy()
    gb, cnt, fst = gboxes.cpu().numpy(), count.cpu().numpy(), first.cpu().numpy()
    pred_boxes = list(pb)
    gt = []
    for si in range(len(sizes)):
        a, b = owner_off[si], owner_off[si + 1]
        f = fst[a:b].copy()
        f[f >= 0] -= scan_off[si]
        gt.append((gb[a:b], cnt[a:b], f))
    return pred_boxes, gt


def instance_boxes(coords, masks, instance_labels, device=None):
    """Boxes of every scan's prediction masks and GT instances, as eval_det.py's ``__main__`` forms
    them.  coords: per scan [n, 3]; masks: per scan a list of masks (RLE dicts or dense arrays, nonzero =
    in); instance_labels: per scan [n] (-100 or any value outside [0, max] ignored).
    -> (per scan [n_masks, 6] fp64, per scan (GT boxes [k, 6] fp64 with k = max label + 1, point counts
    [k], first point index [k] (-1: no points))).  A mask without points raises ValueError, as
    coords[mask].min(0) does."""
    assert len(coords) == len(masks) == len(instance_labels)
    runs = []
    for c, ms, lab in zip(coords, masks, instance_labels):
        n = int(c.shape[0])
        assert tuple(c.shape) == (n, 3) and tuple(lab.shape) == (n,), 'coords [n, 3] and labels [n] per scan'
        scan_runs = []
        for m in ms:
            s, ln = _runs_of(m, n)
            s, ln = np.asarray(s, np.int64), np.asarray(ln, np.int64)
            if int(ln.sum()) == 0:
                raise ValueError('zero-size array to reduction operation minimum which has no identity')
            if (s < 0).any() or (ln < 0).any() or (s + ln > n).any():
                raise ValueError('mask runs outside the scan')
            scan_runs.append((s, ln))
        runs.append(scan_runs)
    res = None
    if use_device(device):
        res = _boxes_device(coords, runs, instance_labels, device)
    if res is None:
        res = _boxes_numpy(coords, runs, instance_labels)
    pred_boxes, gt = res
    out, o = [], 0
    for scan_runs in runs:
        out.append(np.asarray(pred_boxes[o:o + len(scan_runs)], np.float64).reshape(-1, 6))
        o += len(scan_runs)
    return out, gt


def oriented_instance_boxes(coords, masks, instance_labels, yaw_steps=90, refine=0, backend='auto'):
    """``instance_boxes`` with yaw-oriented boxes: every scan's prediction masks and GT instances go
    through ``describe_instances`` (the enclosing rectangle of least area over ``yaw_steps`` directions
    times the z range, float32 coordinates).  The GT owners are ``instance_labels == i`` for i in
    range(max + 1), as in ``instance_boxes``.
    -> (per scan obb [n_masks, 7] fp64 = (cx, cy, cz, du, dv, dz, theta), per scan (GT obb [k, 7], point
    counts [k], first point index [k] (-1: no points))).  A mask without points raises ValueError; an
    owner without points has a NaN box and count 0, which ``evaluate_box_ap`` turns into the reference's
    IndexError."""
    from ..util.objects import describe_instances
    assert len(coords) == len(masks) == len(instance_labels)
    out, gt = [], []
    for c, ms, lab in zip(coords, masks, instance_labels):
        n = int(c.shape[0])
        assert tuple(c.shape) == (n, 3) and tuple(lab.shape) == (n,), 'coords [n, 3] and labels [n] per scan'
        table = describe_instances([dict(pred_mask=m) for m in ms], c, yaw_steps=yaw_steps, refine=refine,
                                   backend=backend)
        if (table['npoint'] == 0).any():
            raise ValueError('zero-size array to reduction operation minimum which has no identity')
        out.append(np.asarray(table['obb'], np.float64).reshape(-1, 7))
        lab = host(lab).astype(np.int64)
        k = max(int(lab.max()) + 1, 0) if lab.size else 0
        owners = [dict(pred_mask=(lab == i)) for i in range(k)]
        gtab = describe_instances(owners, c, yaw_steps=yaw_steps, refine=refine, backend=backend)
        first = np.full(k, -1, np.int64)
        valid = np.flatnonzero((lab >= 0) & (lab < k))
        first[lab[valid][::-1]] = valid[::-1]              # (the lowest point index is written last)
        gt.append((np.asarray(gtab['obb'], np.float64).reshape(-1, 7), gtab['npoint'].astype(np.int64), first))
    return out, gt


def evaluate_box_ap(pred_insts, coords, semantic_labels, instance_labels, class_labels,
                    iou_thresholds=(0.25, 0.5), sem_shift=2, use_07_metric=False, logger=None, device=None,
                    boxes='aabb', mode='3d', yaw_steps=90, refine=0, backend='auto'):
    """Box AP of instance predictions, as the reference's tools/eval_det.py scores them.
    boxes='aabb' (the default): the reference's axis-aligned boxes and ``get_iou``.  boxes='obb':
    yaw-oriented boxes (``oriented_instance_boxes`` with ``yaw_steps`` / ``refine``) and ``get_iou_obb``
    (mode '3d') or ``get_iou_bev`` (mode 'bev'); ``backend`` 'numpy' / 'device' forces both the boxes
    and the matching onto one side, 'auto' leaves the boxes to ``describe_instances`` and the matching
    to ``device``.
    pred_insts: per scan a list of dict(label_id (1-based into class_labels), conf, pred_mask (RLE dict
    or dense array)); coords, semantic_labels, instance_labels: per scan [n, 3] / [n] / [n].
    GT instance i in range(max + 1) takes the class of its first point and counts when that class is
    >= sem_shift (name class_labels[cls - sem_shift]).
    -> {iou_threshold: dict(rec, prec, ap, mAP)} with eval_sphere's dicts."""
    masks = [[p['pred_mask'] for p in preds] for preds in pred_insts]
    iou_func = get_iou
    if boxes == 'aabb':
        pboxes, gts = instance_boxes(coords, masks, instance_labels, device=device)
    elif boxes == 'obb':
        if mode not in ('3d', 'bev') or backend not in ('auto', 'numpy', 'device'):
            raise ValueError(f"mode {mode!r}: '3d' or 'bev'; backend {backend!r}: 'auto', 'numpy' or 'device'")
        iou_func = get_iou_obb if mode == '3d' else get_iou_bev
        device = {'numpy': 'cpu', 'device': 'cuda' if device is None else device, 'auto': device}[backend]
        pboxes, gts = oriented_instance_boxes(coords, masks, instance_labels, yaw_steps, refine, backend)
    else:
        raise ValueError(f"boxes {boxes!r}: 'aabb' or 'obb'")
    pred_all, gt_all = {}, {}
    for si, (preds, boxes, (gb, cnt, first)) in enumerate(zip(pred_insts, pboxes, gts)):
        pred_all[si] = [(class_labels[int(p['label_id']) - 1], boxes[k], float(p['conf']))
                        for k, p in enumerate(preds)]
        sem = host(semantic_labels[si])
        gt = []
        for i in range(len(cnt)):
            if cnt[i] == 0:                        # np.nonzero(inds)[0][0] of an empty instance
                raise IndexError('index 0 is out of bounds for axis 0 with size 0')
            cls_id = int(sem[first[i]])
            if cls_id >= sem_shift:
                gt.append((class_labels[cls_id - sem_shift], gb[i]))
        gt_all[si] = gt
    ths = list(iou_thresholds)
    res = _eval_multi(pred_all, gt_all, ths, use_07_metric, iou_func, device, 'zero') if ths else []
    out = {}
    for t, (rec, prec, ap) in zip(ths, res):
        m = np.mean(list(ap.values()))
        out[t] = dict(rec=rec, prec=prec, ap=ap, mAP=m)
        if logger is not None:
            logger.info(f'box mAP@{t}: {m}')
    return out
