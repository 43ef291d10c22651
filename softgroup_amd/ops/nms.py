"""Greedy non-maximum suppression of instance masks held as bit rows (``sg_mask_nms``, csrc/mask_nms.hip).

The reference has no such step (its ``get_instances`` returns one instance per (proposal, class) pair); the
rules are this project's and are stated in include/softgroup_hip.h:

* order: descending score, the LOWER index first among equal scores (``-0.0 == 0.0``) -- not the ``[::-1]``
  rule of the panoptic fusion and of the pictures;
* a kept mask suppresses every later, not yet suppressed mask of its class (any class when class-agnostic)
  with ``inter / den > thr``, strictly, one double division; ``den = cnt_i + cnt_j - inter`` ('iou') or
  ``min(cnt_i, cnt_j)`` ('min'); ``den == 0`` suppresses nothing; a suppressed mask suppresses nobody.

Bit rows: integer [n, ceil(N / 32)] of 32-bit words, point i = bit i % 32 of word i / 32; bits at and beyond
N are ignored.  CUDA tensors take the HIP kernels (no synchronisation, device results); CPU tensors and numpy
arrays take ``mask_nms_numpy`` on the packed bytes of the same rows.
"""
import numpy as np

__all__ = ['mask_nms', 'mask_nms_numpy', 'mask_bits_from_runs', 'pack_masks', 'MAX_INSTANCES']

MAX_INSTANCES = 16384
_MEASURE = {'iou': 0, 'min': 1}       # softgroup_hip.h: SG_NMS_*

if hasattr(np, 'bitwise_count'):
    _popcount = np.bitwise_count
else:
    _POP8 = np.array([bin(v).count('1') for v in range(256)], dtype=np.uint8)

    def _popcount(a):
        return _POP8[a.view(np.uint8)].reshape(a.shape + (-1, )).sum(-1, dtype=np.uint8) if a.dtype.itemsize > 1 \
            else _POP8[a]


def _measure(measure):
    if measure not in _MEASURE:
        raise ValueError(f"measure {measure!r}: one of 'iou', 'min'")
    return _MEASURE[measure]


def pack_masks(masks, n_points):
    """dense masks [n, N] (bool / 0-1) -> packed uint8 rows [n, 4 * ceil(N / 32)], the bytes of the bit rows"""
    m = np.asarray(masks).reshape(len(masks), n_points) != 0
    width = (n_points + 31) // 32 * 4
    out = np.zeros((m.shape[0], width), dtype=np.uint8)
    if n_points:
        p = np.packbits(m, axis=1, bitorder='little')
        out[:, :p.shape[1]] = p
    return out


def mask_nms_numpy(packed, n_points, scores, labels=None, thr=0.5, measure='iou', class_agnostic=False,
                   return_inter=False):
    """The same rules on packed uint8 rows [n, >= ceil(N / 8)] (little-endian bit order, as the bit rows' bytes).
    Integer work on the packed bytes only: populations by popcount, intersections of a kept mask with the masks
    it may still suppress.  -> (keep uint8 [n], n_keep int, inter int32 [n, n] | None)"""
    meas = _measure(measure)
    thr = float(thr)
    packed = np.asarray(packed)
    n = packed.shape[0]
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    if scores.shape[0] != n:
        raise ValueError(f'{scores.shape[0]} scores for {n} masks')
    if not np.isfinite(scores).all():
        raise ValueError('mask_nms: scores must be finite')
    if labels is None or class_agnostic:
        labels = None
    else:
        labels = np.asarray(labels).reshape(-1).astype(np.int32)
        if labels.shape[0] != n:
            raise ValueError(f'{labels.shape[0]} labels for {n} masks')
    keep = np.zeros(n, dtype=np.uint8)
    if n == 0:
        return keep, 0, (np.zeros((0, 0), np.int32) if return_inter else None)
    nbytes = (n_points + 7) // 8
    rows = np.zeros((n, (nbytes + 7) // 8 * 8), dtype=np.uint8)
    rows[:, :nbytes] = packed.view(np.uint8).reshape(n, -1)[:, :nbytes]
    if n_points & 7:
        rows[:, nbytes - 1] &= (1 << (n_points & 7)) - 1
    rows = rows.view(np.uint64)
    cnt = _popcount(rows).sum(1, dtype=np.int64)
    inter_all = None
    if return_inter:
        inter_all = np.empty((n, n), dtype=np.int32)
        for i in range(n):
            inter_all[i] = _popcount(rows & rows[i]).sum(1, dtype=np.int64)
    order = np.argsort(-scores, kind='stable')        # (-0.0 and 0.0 compare equal: the stable sort keeps the lower index first)
    alive = np.ones(n, dtype=bool)
    for pos in range(n):
        i = order[pos]
        if not alive[i]:
            continue
        keep[i] = 1
        later = order[pos + 1:]
        cand = later[alive[later]]
        if labels is not None:
            cand = cand[labels[cand] == labels[i]]
        if cand.size == 0 or cnt[i] == 0:
            continue
        inter = inter_all[i, cand].astype(np.int64) if inter_all is not None else \
            _popcount(rows[cand] & rows[i]).sum(1, dtype=np.int64)
        den = cnt[i] + cnt[cand] - inter if meas == 0 else np.minimum(cnt[i], cnt[cand])
        ok = den > 0
        hit = np.zeros(cand.size, dtype=bool)
        hit[ok] = inter[ok].astype(np.float64) / den[ok].astype(np.float64) > thr
        alive[cand[hit]] = False
    return keep, int(keep.sum()), inter_all


def mask_bits_from_runs(starts, ends, bounds, n_points):
    """bit rows int32 [n, ceil(N / 32)] on the device from CUDA int32 starts / exclusive ends and int64 bounds
    [n + 1] (``sg_mask_bits_from_runs``: ascending, disjoint runs; runs of mask k = bounds[k] .. bounds[k+1])"""
    import torch

    from .. import _lib as L
    n = bounds.numel() - 1
    words = (int(n_points) + 31) // 32
    bits = torch.empty((n, words), dtype=torch.int32, device=starts.device)
    assert starts.dtype == ends.dtype == torch.int32 and bounds.dtype == torch.int64
    starts, ends, bounds = starts.contiguous(), ends.contiguous(), bounds.contiguous()
    L.check(L.lib().sg_mask_bits_from_runs(L.ptr(starts), L.ptr(ends), L.ptr(bounds), starts.numel(), n,
                                           int(n_points), L.ptr(bits), L.stream()), 'sg_mask_bits_from_runs')
    return bits


def nms_params(nms):
    """(thr, measure, class_agnostic) of a ``test_cfg.nms`` entry (dict or attribute object)"""
    get = nms.get if isinstance(nms, dict) else (lambda k, d=None: getattr(nms, k, d))
    thr, measure = float(get('thr', 0.5)), get('measure', 'iou')
    _measure(measure)
    return thr, measure, bool(get('class_agnostic', False))


def nms_keep_rows(bits_ptr, labels, n, n_points, conf, nms, device):
    """keep flags (numpy bool [n]) of the bit rows at ``bits_ptr``; conf: host float32 [n]; labels: tensor or address"""
    import torch
    thr, measure, agnostic = nms_params(nms)
    scores = torch.from_numpy(np.ascontiguousarray(conf, dtype=np.float32)).to(device)
    keep, _, _ = nms_device_raw(bits_ptr, n, n_points, scores, labels, thr, measure, agnostic, False, device)
    return keep.cpu().numpy().astype(bool)


def nms_device_raw(bits_ptr, n, n_points, scores, labels, thr, measure, class_agnostic, return_inter, device):
    """``sg_mask_nms`` on rows at a raw device address (the scan's arena) -> (keep, n_keep, inter | None), CUDA"""
    import torch

    from .. import _lib as L
    lib = L.lib()
    nb = lib.sg_mask_nms_workspace_bytes(int(n), int(n_points))
    if nb == 0:
        raise L.SoftGroupHipError(f'mask_nms: {n} masks over {n_points} points: outside the supported range '
                                  f'(at most {MAX_INSTANCES} masks, fewer than 2**31 points)')
    keep = torch.empty(n, dtype=torch.uint8, device=device)
    n_keep = torch.empty(1, dtype=torch.int32, device=device)
    inter = torch.empty((n, n), dtype=torch.int32, device=device) if return_inter else None
    ws = L.workspace(nb, device)
    if not (labels is None or isinstance(labels, int)):      # (a tensor, or a raw address inside the scan's arena)
        labels = L.ptr(labels)
    L.check(lib.sg_mask_nms(bits_ptr, int(n), int(n_points), L.ptr(scores), labels, float(thr),
                            _measure(measure), int(bool(class_agnostic)), L.ptr(keep), L.ptr(n_keep), L.ptr(inter),
                            L.ptr(ws), ws.numel(), L.stream()), 'sg_mask_nms')
    return keep, n_keep, inter


def mask_nms(bits, n_points, scores, labels=None, thr=0.5, measure='iou', class_agnostic=False, return_inter=False):
    """-> (keep uint8 [n], n_keep int32 [1]) and, with ``return_inter``, inter int32 [n, n] (populations on the
    diagonal), on the device of ``bits``.  CUDA inputs: HIP kernels, nothing synchronises.  CPU inputs: numpy."""
    import torch
    _measure(measure)
    n_points = int(n_points)
    words = (n_points + 31) // 32
    if not torch.is_tensor(bits):
        bits = torch.from_numpy(np.ascontiguousarray(np.asarray(bits)).view(np.int32))
    if bits.dim() != 2 or bits.element_size() != 4 or bits.is_floating_point() or bits.size(1) != words:
        raise ValueError(f'bits: an integer tensor [n, {words}] of 32-bit words')
    n = bits.size(0)
    scores = torch.as_tensor(scores)
    if scores.numel() != n or (labels is not None and torch.as_tensor(labels).numel() != n):
        raise ValueError(f'scores / labels must have one entry per mask ({n})')
    if not bits.is_cuda:
        packed = bits.contiguous().numpy().view(np.uint8).reshape(n, words * 4)
        keep, n_keep, inter = mask_nms_numpy(packed, n_points, scores.detach().cpu().numpy(),
                                             None if labels is None else torch.as_tensor(labels).cpu().numpy(),
                                             thr, measure, class_agnostic, return_inter)
        out = (torch.from_numpy(keep), torch.tensor([n_keep], dtype=torch.int32))
        return out + (torch.from_numpy(inter), ) if return_inter else out
    dev = bits.device
    bits = bits.contiguous()
    scores = scores.to(dev, torch.float32).reshape(-1).contiguous()
    if labels is not None:
        labels = torch.as_tensor(labels).to(dev, torch.int32).reshape(-1).contiguous()
    keep, n_keep, inter = nms_device_raw(bits.data_ptr() if bits.numel() else None, n, n_points, scores, labels, thr,
                                         measure, class_agnostic, return_inter, dev)
    return (keep, n_keep, inter) if return_inter else (keep, n_keep)
