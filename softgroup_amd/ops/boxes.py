"""Yaw-oriented 3D boxes against each other (csrc/box_ops.hip): the IoU of two boxes, the IoU matrix of two box lists
and greedy box NMS.  The reference has no counterpart; the rules are this project's and are stated in
include/softgroup_hip.h.  Everything below is ONE IEEE double operation per written operation, in the association
written, without contraction.

box rows
  8 doubles ``(cx, cy, cz, du, dv, dz, c, s)``; ``boxes8`` makes them from ``obb`` rows ``(cx, cy, cz, du, dv, dz,
  theta)`` with ``(c, s) = ops.objects._cos_sin(theta)``, once, on the host, for both backends.  ``du`` lies along
  ``(c, s)``, ``dv`` along ``(-s, c)``.  A row with an entry that is not finite or with a negative extent raises
  ``ValueError`` on both backends.
rectangle intersection ``area(a, b)``: a is clipped in b's frame (the arguments are not interchangeable at the last bit)
  1. ``hua = 0.5 * du_a``, ``hva = 0.5 * dv_a``;
  2. corners k = 0 .. 3 with signs (su, sv) = (-,-), (+,-), (+,+), (-,+): ``u = su * hua``, ``v = sv * hva``,
     ``x = cx_a + (u * c_a - v * s_a)``, ``y = cy_a + (u * s_a + v * c_a)``;
  3. ``dx = x - cx_b``, ``dy = y - cy_b``, ``p = (dx * c_b + dy * s_b, dy * c_b - dx * s_b)``;
  4. Sutherland-Hodgman against (axis 0, +, hub), (axis 0, -, hub), (axis 1, +, hvb), (axis 1, -, hvb), ``hub = 0.5 *
     du_b``, ``hvb = 0.5 * dv_b``: for the edges ``(P[i], P[(i + 1) % n])``, i ascending, ``dp = h - sign * p[axis]``,
     ``dq`` likewise; inside is ``d >= 0`` (a NaN is outside); p is emitted when inside; when exactly one end is
     inside, ``t = dp / (dp - dq)`` and ``r = p + t * (q - p)`` per coordinate, the clipped coordinate set to exactly
     ``sign * h``, is emitted as well.  An empty polygon ends the walk with area 0.  A convex polygon gains at most
     one vertex per plane, so 8 slots hold it; an emit into a full polygon is dropped (never reached by valid boxes:
     the guard that keeps every store inside the 8 slots whatever the input);
  5. fewer than 3 vertices: area 0;
  6. ``S = +0.0``; for i = 1 .. n-2 ascending ``S = S + ((x_i - x0) * (y_{i+1} - y0) - (x_{i+1} - x0) * (y_i -
     y0))``; ``area = 0.5 * abs(S)``.
IoU
  '3d': ``zlo = max(cz_a - 0.5 * dz_a, cz_b - 0.5 * dz_b)``, ``zhi = min(cz_a + 0.5 * dz_a, cz_b + 0.5 * dz_b)`` (``max(x,
  y) = x if x > y else y``, ``min(x, y) = x if x < y else y``), ``h = zhi - zlo``; ``h > 0`` false: 0.0, before any
  clipping.  ``A = area(a, b)``; ``A > 0`` false: 0.0.  ``inter = A * h``, ``va = (du_a * dv_a) * dz_a``, ``vb``
  likewise, ``uni = (va + vb) - inter``; ``uni > 0`` false: 0.0, else ``inter / uni``.  'bev': the same without z,
  ``uni = (du_a * dv_a + du_b * dv_b) - A``.  Not clamped: a box against itself gives 1 within a few ulps.  Touching
  boxes and boxes of zero extent give exactly 0.  Thresholds compare strictly, ``iou > thr``.
NMS (the order and the loop of ``mask_nms``)
  descending float32 score, the LOWER index first among equal scores; a kept box suppresses every later, not yet
  suppressed box of its label (any label when class-agnostic) with ``iou > thr``; a suppressed box suppresses nobody.
  The pair of original indices i < j is evaluated as ``iou(box_i, box_j)``.

CUDA tensors take the HIP kernels, numpy arrays the ``*_numpy`` twins, which are the definition the device results are
held to byte for byte.  ``obb_iou_pair`` is the scalar form, written to be read; ``box_iou_numpy`` equals it byte for
byte.
"""
import numpy as np

from ._args import _is_cuda, choose_backend

__all__ = ['auto_backend', 'boxes8', 'obb_iou_pair', 'box_iou', 'box_iou_numpy', 'box_nms', 'box_nms_numpy',
           'MAX_NMS_BOXES', 'MAX_PAIRS', 'FLAG_INVALID']

MAX_NMS_BOXES = 16384        # kBoxMaxNms
MAX_PAIRS = 2**30            # 1 << kBoxMaxPairsLog2
FLAG_INVALID = 1             # SG_BOX_FLAG_INVALID
_MODE = {'3d': 0, 'bev': 1}  # SG_BOX_IOU_*
_SIGNS = ((-1.0, -1.0), (1.0, -1.0), (1.0, 1.0), (-1.0, 1.0))
_CHUNK = 1 << 16             # pairs per pass of the vectorised twin

# what backend='auto' means with a GPU present -- the single place to change.  It follows profiles/box_ops_bench.txt
# (tools/box_ops_bench.py; wall, MI355X, host arrays in, host result out), where the device is ahead of the vectorised
# twin on every set by far more than the spread of the five repetitions: the matrix of 100 / 300 / 1000 boxes 0.14 /
# 0.19 / 0.88 ms against 9.0 / 103 / 2029 ms, NMS 0.13 / 0.30 / 0.27 ms against 1.3 [1.0 .. 1.7] / 8.9 / 32 ms, the
# match of 312 images x 18 classes 15 ms against 1181 ms.
_AUTO = {'iou': 'device', 'nms': 'device', 'match': 'device'}


def auto_backend(backend, what='iou'):
    """'device' or 'numpy' for one of the operations of ``_AUTO``"""
    return choose_backend(backend, _AUTO[what])


def _mode(mode):
    if mode not in _MODE:
        raise ValueError(f"mode {mode!r}: one of '3d', 'bev'")
    return _MODE[mode]


def boxes8(obb):
    """obb float [n, 7] = (cx, cy, cz, du, dv, dz, theta), or an ``ObjectTable`` -> box rows float64 [n, 8]"""
    from .objects import _cos_sin
    obb = np.asarray(obb['obb'] if isinstance(obb, dict) else obb, dtype=np.float64)
    if obb.ndim == 1 and obb.size == 7:
        obb = obb.reshape(1, 7)
    if obb.ndim != 2 or obb.shape[1] != 7:
        raise ValueError('obb: an array [n, 7]')
    return np.ascontiguousarray(np.concatenate([obb[:, :6], _cos_sin(obb[:, 6])], axis=1))


def _rows8(boxes, what='boxes'):
    boxes = np.ascontiguousarray(np.asarray(boxes, dtype=np.float64))
    if boxes.ndim == 1 and boxes.size == 8:
        boxes = boxes.reshape(1, 8)
    if boxes.ndim != 2 or boxes.shape[1] != 8:
        raise ValueError(f'{what}: box rows [n, 8]')
    return boxes


def _invalid(rows):
    return ~(np.isfinite(rows).all(1) & (rows[:, 3:6] >= 0).all(1))


def _check(rows, what):
    if _invalid(rows).any():
        raise ValueError(f'{what}: a box with an entry that is not finite or with a negative extent')


# ---- the scalar definition ---------------------------------------------------------------------------------------------
def _clip_pair(a, b):
    """the polygon of rectangle a inside rectangle b, in b's frame: a list of (x, y)"""
    cxa, cya, _, dua, dva, _, ca, sa = a
    cxb, cyb, _, dub, dvb, _, cb, sb = b
    hua, hva = 0.5 * dua, 0.5 * dva
    poly = []
    for su, sv in _SIGNS:
        u, v = su * hua, sv * hva
        x = cxa + (u * ca - v * sa)
        y = cya + (u * sa + v * ca)
        dx, dy = x - cxb, y - cyb
        poly.append((dx * cb + dy * sb, dy * cb - dx * sb))
    hub, hvb = 0.5 * dub, 0.5 * dvb
    for axis, sign, h in ((0, 1.0, hub), (0, -1.0, hub), (1, 1.0, hvb), (1, -1.0, hvb)):
        out = []
        n = len(poly)
        for i in range(n):
            p, q = poly[i], poly[(i + 1) % n]
            dp, dq = h - sign * p[axis], h - sign * q[axis]
            p_in, q_in = bool(dp >= 0), bool(dq >= 0)
            if p_in and len(out) < 8:
                out.append(p)
            if p_in != q_in and len(out) < 8:
                t = dp / (dp - dq)
                r = [p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])]
                r[axis] = sign * h
                out.append(tuple(r))
        poly = out
        if not poly:
            break
    return poly


def _area_pair(a, b):
    poly = _clip_pair(a, b)
    n = len(poly)
    if n < 3:
        return 0.0
    x0, y0 = poly[0]
    acc = 0.0
    for i in range(1, n - 1):
        acc = acc + ((poly[i][0] - x0) * (poly[i + 1][1] - y0) - (poly[i + 1][0] - x0) * (poly[i][1] - y0))
    return 0.5 * abs(acc)


def obb_iou_pair(a, b, mode='3d'):
    """IoU of two box rows (8 numbers each): the definition, one pair at a time -> a Python float"""
    m = _mode(mode)
    with np.errstate(all='ignore'):
        a = [float(v) for v in np.asarray(a, dtype=np.float64).reshape(8)]
        b = [float(v) for v in np.asarray(b, dtype=np.float64).reshape(8)]
        _check(np.array([a, b]), 'obb_iou_pair')
        h = 1.0
        if m == 0:
            lo_a, lo_b = a[2] - 0.5 * a[5], b[2] - 0.5 * b[5]
            hi_a, hi_b = a[2] + 0.5 * a[5], b[2] + 0.5 * b[5]
            zlo = lo_a if lo_a > lo_b else lo_b
            zhi = hi_a if hi_a < hi_b else hi_b
            h = zhi - zlo
            if not h > 0:
                return 0.0
        area = _area_pair(a, b)
        if not area > 0:
            return 0.0
        if m == 0:
            inter = area * h
            uni = ((a[3] * a[4]) * a[5] + (b[3] * b[4]) * b[5]) - inter
        else:
            inter = area
            uni = (a[3] * a[4] + b[3] * b[4]) - area
        if not uni > 0:
            return 0.0
        return float(np.float64(inter) / np.float64(uni))


# ---- the vectorised twin -----------------------------------------------------------------------------------------------
def _area_rows(A, B):
    """area(a_k, b_k) for the rows of A, B [m, 8]: padded 8-slot polygons (a ninth slot takes what is not emitted)"""
    m = A.shape[0]
    rows = np.arange(m)
    hua, hva = 0.5 * A[:, 3], 0.5 * A[:, 4]
    P = np.zeros((m, 9, 2))
    for k, (su, sv) in enumerate(_SIGNS):
        u, v = su * hua, sv * hva
        x = A[:, 0] + (u * A[:, 6] - v * A[:, 7])
        y = A[:, 1] + (u * A[:, 7] + v * A[:, 6])
        dx, dy = x - B[:, 0], y - B[:, 1]
        P[:, k, 0] = dx * B[:, 6] + dy * B[:, 7]
        P[:, k, 1] = dy * B[:, 6] - dx * B[:, 7]
    n = np.full(m, 4, dtype=np.int64)
    hub, hvb = 0.5 * B[:, 3], 0.5 * B[:, 4]
    for axis, sign, h in ((0, 1.0, hub), (0, -1.0, hub), (1, 1.0, hvb), (1, -1.0, hvb)):
        Q = np.zeros((m, 9, 2))
        cnt = np.zeros(m, dtype=np.int64)
        for i in range(8):
            act = i < n
            if not act.any():
                break
            p = P[:, i, :]
            q = P[rows, np.where(i + 1 < n, i + 1, 0), :]
            dp, dq = h - sign * p[:, axis], h - sign * q[:, axis]
            p_in, q_in = dp >= 0, dq >= 0
            emit = act & p_in & (cnt < 8)
            Q[rows, np.where(emit, cnt, 8), :] = p
            cnt = cnt + emit
            emit = act & (p_in != q_in) & (cnt < 8)
            t = dp / (dp - dq)
            r = p + t[:, None] * (q - p)
            r[:, axis] = sign * h
            Q[rows, np.where(emit, cnt, 8), :] = r
            cnt = cnt + emit
        P, n = Q, cnt
    x0, y0 = P[:, 0, 0], P[:, 0, 1]
    acc = np.zeros(m)
    for i in range(1, 7):
        term = (P[:, i, 0] - x0) * (P[:, i + 1, 1] - y0) - (P[:, i + 1, 0] - x0) * (P[:, i, 1] - y0)
        acc = np.where(i <= n - 2, acc + term, acc)
    return np.where(n >= 3, 0.5 * np.abs(acc), 0.0)


def _iou_rows(A, B, m):
    """iou(a_k, b_k) for valid rows A, B [k, 8] -> float64 [k]"""
    out = np.zeros(A.shape[0])
    with np.errstate(all='ignore'):
        for at in range(0, A.shape[0], _CHUNK):
            a, b = A[at:at + _CHUNK], B[at:at + _CHUNK]
            if m == 0:
                lo_a, lo_b = a[:, 2] - 0.5 * a[:, 5], b[:, 2] - 0.5 * b[:, 5]
                hi_a, hi_b = a[:, 2] + 0.5 * a[:, 5], b[:, 2] + 0.5 * b[:, 5]
                h = np.where(hi_a < hi_b, hi_a, hi_b) - np.where(lo_a > lo_b, lo_a, lo_b)
                live = np.flatnonzero(h > 0)
            else:
                live = np.arange(a.shape[0])
            if live.size == 0:
                continue
            a, b = a[live], b[live]
            area = _area_rows(a, b)
            if m == 0:
                inter = area * h[live]
                uni = ((a[:, 3] * a[:, 4]) * a[:, 5] + (b[:, 3] * b[:, 4]) * b[:, 5]) - inter
            else:
                inter = area
                uni = (a[:, 3] * a[:, 4] + b[:, 3] * b[:, 4]) - area
            out[at + live] = np.where((area > 0) & (uni > 0), inter / uni, 0.0)
    return out


def box_iou_numpy(a, b, mode='3d'):
    """box rows a [n_a, 8], b [n_b, 8] -> float64 [n_a, n_b], ``[i, j] = iou(a_i, b_j)``"""
    m = _mode(mode)
    a, b = _rows8(a, 'a'), _rows8(b, 'b')
    _check(a, 'box_iou'), _check(b, 'box_iou')
    n_a, n_b = a.shape[0], b.shape[0]
    if n_a == 0 or n_b == 0:
        return np.zeros((n_a, n_b))
    out = np.empty((n_a, n_b))
    step = max(1, _CHUNK // n_b)
    for at in range(0, n_a, step):
        rows = a[at:at + step]
        out[at:at + step] = _iou_rows(np.repeat(rows, n_b, axis=0), np.tile(b, (rows.shape[0], 1)),
                                      m).reshape(rows.shape[0], n_b)
    return out


def _flags_raise(flags, what):
    if int(flags) & FLAG_INVALID:
        raise ValueError(f'{what}: a box with an entry that is not finite or with a negative extent')


def _rows8_device(t, what):
    import torch
    if t.dim() != 2 or t.size(1) != 8:
        raise ValueError(f'{what}: box rows [n, 8]')
    return t.detach().to(torch.float64).contiguous()


def box_iou(a, b, mode='3d'):
    """IoU matrix [n_a, n_b] of two lists of box rows.  CUDA tensors: ``sg_box_iou``, a CUDA float64 tensor comes back
    (the flag word is read once the kernels are enqueued; invalid boxes raise ``ValueError``).  Anything else:
    ``box_iou_numpy``."""
    if not (_is_cuda(a) and _is_cuda(b)):
        from ._args import _host
        return box_iou_numpy(_host(a), _host(b), mode)
    import torch

    from .. import _lib as L
    m = _mode(mode)
    a, b = _rows8_device(a, 'a'), _rows8_device(b, 'b')
    n_a, n_b = a.size(0), b.size(0)
    if n_a * n_b > MAX_PAIRS:
        raise L.SoftGroupHipError(f'box_iou: {n_a} x {n_b} boxes: outside the supported range (at most 2**30 pairs)')
    with torch.cuda.device(a.device):
        out = torch.empty((n_a, n_b), dtype=torch.float64, device=a.device)
        flags = torch.zeros(1, dtype=torch.int32, device=a.device)
        L.check(L.lib().sg_box_iou(L.ptr(a), n_a, L.ptr(b), n_b, m, L.ptr(out), L.ptr(flags), L.stream()),
                'sg_box_iou')
        _flags_raise(flags.item(), 'box_iou')
    return out


# ---- NMS ---------------------------------------------------------------------------------------------------------------
def _nms_args(n, scores, labels, class_agnostic):
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    if scores.shape[0] != n:
        raise ValueError(f'{scores.shape[0]} scores for {n} boxes')
    if not np.isfinite(scores).all():
        raise ValueError('box_nms: scores must be finite')
    if labels is None or class_agnostic:
        labels = None
    else:
        labels = np.asarray(labels).reshape(-1).astype(np.int32)
        if labels.shape[0] != n:
            raise ValueError(f'{labels.shape[0]} labels for {n} boxes')
    return scores, labels


def box_nms_numpy(boxes, scores, labels=None, thr=0.25, mode='3d', class_agnostic=False, return_iou=False):
    """-> (keep uint8 [n], n_keep int, iou float64 [n, n] | None).  ``iou`` is symmetric: ``[i, j] = [j, i] =
    iou(box_i, box_j)`` for i <= j, every pair, whatever the labels."""
    m = _mode(mode)
    thr = float(thr)
    boxes = _rows8(boxes)
    n = boxes.shape[0]
    scores, labels = _nms_args(n, scores, labels, class_agnostic)
    _check(boxes, 'box_nms')
    keep = np.zeros(n, dtype=np.uint8)
    if n == 0:
        return keep, 0, (np.zeros((0, 0)) if return_iou else None)
    i, j = np.triu_indices(n, 0 if return_iou else 1)
    if labels is not None and not return_iou:
        same = labels[i] == labels[j]
        i, j = i[same], j[same]
    upper = np.zeros((n, n))
    upper[i, j] = _iou_rows(boxes[i], boxes[j], m)
    order = np.argsort(-scores, kind='stable')        # (-0.0 and 0.0 compare equal: the stable sort keeps the lower index first)
    alive = np.ones(n, dtype=bool)
    for pos in range(n):
        k = order[pos]
        if not alive[k]:
            continue
        keep[k] = 1
        later = order[pos + 1:]
        cand = later[alive[later]]
        if labels is not None:
            cand = cand[labels[cand] == labels[k]]
        if cand.size:
            alive[cand[upper[np.minimum(k, cand), np.maximum(k, cand)] > thr]] = False
    full = None
    if return_iou:
        full = upper + upper.T
        full[np.arange(n), np.arange(n)] = upper[np.arange(n), np.arange(n)]
    return keep, int(keep.sum()), full


def box_nms(boxes, scores, labels=None, thr=0.25, mode='3d', class_agnostic=False, return_iou=False):
    """-> (keep uint8 [n], n_keep) and, with ``return_iou``, iou float64 [n, n].  CUDA ``boxes``: ``sg_box_nms``, CUDA
    tensors come back, ``n_keep`` int32 [2] = (the count, the flag word -- ``FLAG_INVALID`` when a box is not valid,
    the other outputs then mean nothing); nothing synchronises.  Anything else: ``box_nms_numpy`` (``n_keep`` an
    int)."""
    if not _is_cuda(boxes):
        from ._args import _host
        out = box_nms_numpy(_host(boxes), _host(scores), None if labels is None else _host(labels), thr, mode,
                            class_agnostic, return_iou)
        return out if return_iou else out[:2]
    import torch

    from .. import _lib as L
    m = _mode(mode)
    thr = float(thr)
    boxes = _rows8_device(boxes, 'boxes')
    n, dev = boxes.size(0), boxes.device
    scores = torch.as_tensor(scores).to(dev, torch.float32).reshape(-1).contiguous()
    if scores.numel() != n or (labels is not None and torch.as_tensor(labels).numel() != n):
        raise ValueError(f'scores / labels must have one entry per box ({n})')
    if labels is not None:
        labels = torch.as_tensor(labels).to(dev, torch.int32).reshape(-1).contiguous()
    lib = L.lib()
    nb = lib.sg_box_nms_workspace_bytes(n)
    if nb == 0:
        raise L.SoftGroupHipError(f'box_nms: {n} boxes: outside the supported range (at most {MAX_NMS_BOXES})')
    with torch.cuda.device(dev):
        keep = torch.empty(n, dtype=torch.uint8, device=dev)
        n_keep = torch.empty(2, dtype=torch.int32, device=dev)
        iou = torch.empty((n, n), dtype=torch.float64, device=dev) if return_iou else None
        ws = L.workspace(nb, dev)
        L.check(lib.sg_box_nms(L.ptr(boxes), n, L.ptr(scores), L.ptr(labels), thr, m, int(bool(class_agnostic)),
                               L.ptr(keep), L.ptr(n_keep), L.ptr(iou), L.ptr(ws), ws.numel(), L.stream()),
                'sg_box_nms')
    return (keep, n_keep, iou) if return_iou else (keep, n_keep)
