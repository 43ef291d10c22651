"""Semantic accuracy / mIoU and offset MAE, the point-wise half of the evaluation tools/test.py runs
for ``eval_tasks: ['semantic']``.  Same signatures, return values and log lines as the
reference's softgroup/evaluation/point_wise_eval.py:4-44; ``logger=None`` means no logging, and
``device`` chooses the path as in ``ScanNetEval`` (None: the GPU when one is available).

On the GPU every scan goes to the device once and ``sg_eval_class_tally`` produces, in one pass, the
per-class seen / positive / correct counts of the valid points and the masked |offset| sum; mIoU and
accuracy follow from the integer counts exactly (U = seen + positive - correct).  Inputs the kernel
cannot represent exactly (float labels, a ground-truth class outside [0, SG_EVAL_MAX_CLASSES),
non-float32 offsets) take the numpy path, which restates the reference's arithmetic.
"""
import numpy as np

MAX_CLASSES = 1024               # SG_EVAL_MAX_CLASSES
_I32, _I64, _U32 = 0, 1, 2       # SG_EVAL_I32 / _I64 / _U32
_BAD_GT, _BAD_PRED, _BAD_INST = 1, 2, 4
_CHUNK_POINTS = 1 << 22


# ------------------------------------------------------------------ shared by the device paths
def use_device(device):
    import torch
    return torch.cuda.is_available() if device is None else str(device).startswith('cuda')


def host(a):
    """numpy view of a numpy array or a (possibly device) torch tensor"""
    import torch
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().numpy()
    return np.asarray(a)


def _dtype_name(a):
    import torch
    if isinstance(a, torch.Tensor):
        return {torch.int8: 'int8', torch.uint8: 'uint8', torch.int16: 'int16', torch.int32: 'int32',
                torch.int64: 'int64', torch.float32: 'float32'}.get(a.dtype, str(a.dtype))
    return np.asarray(a).dtype.name


def label_kind(arrs):
    """kernel kind for a list of label arrays, or None (not representable: numpy path)"""
    names = {_dtype_name(a) for a in arrs}
    if not names:
        return _I64
    if names == {'uint32'}:
        return _U32
    if names <= {'int8', 'uint8', 'int16', 'uint16', 'int32'}:
        return _I32
    if names <= {'int8', 'uint8', 'int16', 'uint16', 'int32', 'int64', 'uint32'}:
        return _I64
    return None


def stage(arrs, kind, dev, width=1):
    """the arrays laid end to end in one fresh (256-byte aligned) device buffer of the kind's type"""
    import torch
    n = sum(int(a.shape[0]) for a in arrs)
    if kind == 'f32':
        buf = torch.empty(n * width, dtype=torch.float32, device=dev)
    else:
        buf = torch.empty(n, dtype=torch.int64 if kind == _I64 else torch.int32, device=dev)
    o = 0
    for a in arrs:
        m = int(a.shape[0]) * width
        if not isinstance(a, torch.Tensor):
            a = np.ascontiguousarray(a)
            if kind == _U32:
                a = a.view(np.int32)                     # the bits; the kernel reads them unsigned
            elif a.dtype == np.uint32:
                a = a.astype(np.int64)
            a = torch.from_numpy(a)
        buf[o:o + m].copy_(a.reshape(-1))
        o += m
    return buf


def chunks(sizes, max_points, max_scans=0xFFFF):
    """[first, last) scan ranges of at most max_points points (one scan may exceed it alone) and at
    most max_scans scans each"""
    out, first, acc = [], 0, 0
    for i, s in enumerate(sizes):
        if i > first and (acc + s > max_points or i - first == max_scans):
            out.append((first, i))
            first, acc = i, 0
        acc += s
    if sizes:
        out.append((first, len(sizes)))
    return out


def _is_int(x):
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool)


def _device_pass(pred_list, gt_list, ignore_label, device, inst_list=None, opred_list=None, ogt_list=None):
    """-> (seen, positive, correct) int64 [MAX_CLASSES] (None without pred_list), offset |d| sum,
    offset point count; or None when the inputs need the numpy path"""
    import torch
    from .. import _lib as L
    if not _is_int(ignore_label) or not -2**63 <= int(ignore_label) < 2**63:
        return None
    with_cls = pred_list is not None
    with_off = opred_list is not None
    groups = []
    if with_cls:
        pk, gk = label_kind(pred_list), label_kind(gt_list)
        if pk is None or gk is None or len(pred_list) != len(gt_list):
            return None
        groups += [pred_list, gt_list]
    if with_off:
        ik = label_kind(inst_list)
        if ik is None or len(opred_list) != len(ogt_list) or len(opred_list) != len(inst_list):
            return None
        for a in list(opred_list) + list(ogt_list):
            if _dtype_name(a) != 'float32' or tuple(a.shape[1:]) != (3,):
                return None
        groups += [inst_list, opred_list, ogt_list]
    sizes = [int(a.shape[0]) for a in groups[0]]
    for g in groups[1:]:
        if [int(a.shape[0]) for a in g] != sizes:
            return None
    dev = torch.device('cuda' if device is None else device)
    with torch.cuda.device(dev):
        out = torch.zeros(3 * MAX_CLASSES + 2, dtype=torch.int64, device=dev)   # tallies | count | flags
        off_sum = torch.zeros(1, dtype=torch.float64, device=dev)
        for a, b in chunks(sizes, _CHUNK_POINTS):
            n = sum(sizes[a:b])
            pred = stage(pred_list[a:b], pk, dev) if with_cls else None
            gt = stage(gt_list[a:b], gk, dev) if with_cls else None
            inst = stage(inst_list[a:b], ik, dev) if with_off else None
            op = stage(opred_list[a:b], 'f32', dev, 3) if with_off else None
            og = stage(ogt_list[a:b], 'f32', dev, 3) if with_off else None
            ws = L.workspace(L.lib().sg_eval_tally_workspace_bytes(n), dev)
            L.check(L.lib().sg_eval_class_tally(
                L.ptr(pred), pk if with_cls else 0, L.ptr(gt), gk if with_cls else 0, n, int(ignore_label), 0,
                MAX_CLASSES, L.ptr(out) if with_cls else None, L.ptr(inst), ik if with_off else 0, L.ptr(op),
                L.ptr(og), L.ptr(off_sum), out.data_ptr() + 8 * 3 * MAX_CLASSES,
                out.data_ptr() + 8 * (3 * MAX_CLASSES + 1), L.ptr(ws), ws.numel(), L.stream()), 'sg_eval_class_tally')
        res = out.cpu().numpy()
        s = off_sum.cpu().numpy()[0]
    if with_cls and int(res[-1]) & _BAD_GT:
        return None
    t = res[:3 * MAX_CLASSES].reshape(3, MAX_CLASSES)
    return (t if with_cls else None), s, res[3 * MAX_CLASSES]


def _log(logger, msg):
    if logger is not None:
        logger.info(msg)


# ------------------------------------------------------------------ the three evaluators
def evaluate_semantic_acc(pred_list, gt_list, ignore_label=-100, logger=None, *, device=None):
    r = _device_pass(pred_list, gt_list, ignore_label, device) if use_device(device) else None
    if r is not None:
        seen, _, correct = r[0]
        correct, whole = np.int64(correct.sum()), np.int64(seen.sum())
    else:
        gt = np.concatenate([host(a) for a in gt_list], axis=0)
        pred = np.concatenate([host(a) for a in pred_list], axis=0)
        assert gt.shape == pred.shape
        valid = gt != ignore_label
        correct = (gt[valid] == pred[valid]).sum()
        whole = valid.sum()
    # correct / whole * 100 with `correct` cast to float (numpy scalars: 0 / 0 is nan, as there)
    acc = correct.astype(float) / whole * 100
    _log(logger, f'Acc: {acc:.1f}')
    return acc


def evaluate_semantic_miou(pred_list, gt_list, ignore_label=-100, logger=None, *, device=None):
    r = _device_pass(pred_list, gt_list, ignore_label, device) if use_device(device) else None
    if r is not None:
        seen, positive, correct = r[0]
        classes = np.flatnonzero(seen > 0)
        inter = correct[classes]
        union = seen[classes] + positive[classes] - inter
    else:
        gt = np.concatenate([host(a) for a in gt_list], axis=0)
        pred = np.concatenate([host(a) for a in pred_list], axis=0)
        valid = gt != ignore_label
        gt, pred = gt[valid], pred[valid]
        assert gt.shape == pred.shape
        classes, gt_idx = np.unique(gt, return_inverse=True)
        gt_idx = gt_idx.reshape(-1)
        hit = gt == pred
        n_gt = np.bincount(gt_idx, minlength=len(classes))
        inter = np.bincount(gt_idx[hit], minlength=len(classes))
        at = np.searchsorted(classes, pred)
        is_cls = at < len(classes)
        is_cls[is_cls] = classes[at[is_cls]] == pred[is_cls]
        n_pred = np.bincount(at[is_cls], minlength=len(classes))
        union = n_gt + n_pred - inter
        keep = classes != ignore_label
        inter, union = inter[keep], union[keep]
    # the mean runs over the classes present in the GROUND TRUTH (np.unique(gt) after the ignore
    # filter), not over all classes; IoU = float(I) / U * 100; np.mean of the list (nan when empty)
    iou_list = [np.int64(i).astype(float) / np.int64(u) * 100 for i, u in zip(inter, union)]
    miou = np.mean(iou_list)
    _log(logger, 'Class-wise mIoU: ' + ' '.join(f'{x:.1f}' for x in iou_list))
    _log(logger, f'mIoU: {miou:.1f}')
    return miou


def evaluate_offset_mae(pred_list, gt_list, gt_instance_list, ignore_label=-100, logger=None, *, device=None):
    r = (_device_pass(None, None, ignore_label, device, gt_instance_list, pred_list, gt_list)
         if use_device(device) else None)
    if r is not None:
        # fp64 sum in a fixed order on the device (numpy sums float32 pairwise: last bits may differ)
        mae = np.float64(r[1]) / np.int64(r[2])
    else:
        gt = np.concatenate([host(a) for a in gt_list], axis=0)
        pred = np.concatenate([host(a) for a in pred_list], axis=0)
        gt_instance = np.concatenate([host(a) for a in gt_instance_list], axis=0)
        # the points whose INSTANCE label is not ignored; divided by their number, not by 3x it
        pos_inds = gt_instance != ignore_label
        mae = np.abs(gt[pos_inds] - pred[pos_inds]).sum() / pos_inds.sum()
    _log(logger, f'Offset MAE: {mae:.3f}')
    return mae
