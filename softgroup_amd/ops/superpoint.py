"""Masks and semantic labels snapped to an over-segmentation, "superpoints" (``sg_superpoint_index``,
``sg_mask_snap``, ``sg_superpoint_vote``, csrc/superpoint.hip).

The reference has no such step.  ScanNet ships an over-segmentation with every scene (``*.segs.json``) and most
pipelines refine their masks and labels on it: the points of one superpoint lie on one smooth surface patch, so a
mask that covers most of a patch takes all of it and a mask that holds a few stray points of a patch gives them up.
The rules are this project's and are stated in include/softgroup_hip.h; the ``*_numpy`` functions are the definition:

* ``sp`` [N]: the superpoint id of every point, arbitrary integers in ``0 .. 2**31 - 2``; ``-1`` = in no superpoint;
  an id below -1 or at or above ``2**31 - 1`` raises ``ValueError``;
* a segment is the set of points with one id; segments are numbered in ascending id order and hold their points in
  ascending index order;
* mask snap: ``inter`` = points of segment s in mask k; the segment is taken when ``inter >= 1`` and
  ``float64(inter) / float64(size) > thr`` (strict); a point in no superpoint keeps its bit; ``'snap'`` gives
  ``taken``, ``'grow'`` ``in | taken``, ``'trim'`` ``in & taken``;
* label vote: per segment the labels in ``0 .. n_classes - 1`` (other than ``ignore_label``) are counted, the class
  with the greatest count wins, the lowest among equal counts, and every point of the segment receives it; a segment
  without a counted label and the points in no superpoint keep their own labels.

Bit rows: integer [n, ceil(N / 32)] of 32-bit words, point i = bit i % 32 of word i / 32; bits at and beyond N are
ignored on input and zero on output.  CUDA tensors take the HIP kernels (one read-back in all: ``meta`` of the index
build), CPU tensors and numpy arrays the numpy twins.
"""
import numpy as np

from ._args import _host, choose_backend

__all__ = ['SuperpointIndex', 'superpoint_index', 'superpoint_index_numpy', 'mask_snap', 'mask_snap_numpy',
           'superpoint_vote', 'superpoint_vote_numpy', 'auto_backend', 'MAX_INSTANCES', 'MAX_CLASSES', 'WALK']

MAX_INSTANCES = 16384
MAX_CLASSES = 256                         # of the vote on the device
WALK = 2048                               # softgroup_hip.h: SG_SUPERPOINT_WALK, the positions one workgroup walks
_MODE = {'snap': 0, 'grow': 1, 'trim': 2}  # softgroup_hip.h: SG_SNAP_*
_ID_END = 2**31 - 1

# what backend='auto' means with a GPU present -- the single place to change.  Set from
# profiles/superpoint_bench.txt (tools/superpoint_bench.py, MI355X), where the device is ahead on both clouds:
# snap_instances 0.7 - 3.2 ms against 146 - 1774 ms, the vote 0.07 - 0.10 ms against 3.5 - 14.8 ms (and the index
# that both need 0.14 - 0.22 ms against 8.3 - 39 ms).
_AUTO = {'snap': 'device', 'vote': 'device'}


def auto_backend(backend, what):
    """'device' or 'numpy' for one of the operations of ``_AUTO``"""
    return choose_backend(backend, _AUTO[what])


def _thr_mode(thr, mode):
    if mode not in _MODE:
        raise ValueError(f"mode {mode!r}: one of 'snap', 'grow', 'trim'")
    thr = float(thr)
    if not (np.isfinite(thr) and 0.0 <= thr <= 1.0):
        raise ValueError(f'thr {thr!r}: a finite number in [0, 1]')
    return thr, mode


def _classes(n_classes):
    if int(n_classes) != n_classes or int(n_classes) < 1:
        raise ValueError(f'n_classes {n_classes!r}: an integer >= 1')
    return int(n_classes)


def _bad_id():
    return ValueError('superpoint ids: integers in 0 .. 2**31 - 2, or -1 for a point in no superpoint')


class SuperpointIndex:
    """The segments of one cloud: ``order`` int32 [n_valid] (the points of segment 0, then of segment 1, ...),
    ``seg_of`` int32 [N] (-1 = none), ``seg_start`` int32 [S + 1]; ``n_points``, ``n_seg``, ``n_valid`` and
    ``max_size`` (the largest segment) on the host.  The arrays are numpy arrays or CUDA tensors."""

    __slots__ = ('n_points', 'n_seg', 'n_valid', 'max_size', 'order', 'seg_of', 'seg_start')

    def __init__(self, n_points, n_seg, n_valid, max_size, order, seg_of, seg_start):
        self.n_points, self.n_seg, self.n_valid, self.max_size = int(n_points), int(n_seg), int(n_valid), int(max_size)
        self.order, self.seg_of, self.seg_start = order, seg_of, seg_start

    @property
    def is_cuda(self):
        return not isinstance(self.seg_of, np.ndarray)

    @property
    def device(self):
        return self.seg_of.device if self.is_cuda else None

    def numpy(self):
        """the same index with numpy arrays (itself when it has them)"""
        if not self.is_cuda:
            return self
        return SuperpointIndex(self.n_points, self.n_seg, self.n_valid, self.max_size, self.order.cpu().numpy(),
                               self.seg_of.cpu().numpy(), self.seg_start.cpu().numpy())

    def cuda(self, device=None):
        """the same index with CUDA tensors on ``device`` (itself when it is there)"""
        import torch
        device = torch.device('cuda' if device is None else device)
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if self.is_cuda:
            if self.seg_of.device == device:
                return self
            arrays = (self.order.to(device), self.seg_of.to(device), self.seg_start.to(device))
        else:
            arrays = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device)
                           for a in (self.order, self.seg_of, self.seg_start))
        return SuperpointIndex(self.n_points, self.n_seg, self.n_valid, self.max_size, *arrays)


# ---- the definitions -------------------------------------------------------------------------------------------------
def superpoint_index_numpy(sp):
    """The definition: ``np.unique`` and a stable argsort -> SuperpointIndex of numpy arrays"""
    sp = _host(sp)
    if sp.ndim != 1 or sp.dtype.kind not in 'iu':
        raise ValueError('superpoint ids: a 1-D integer array, one id per point')
    n = sp.size
    if n and (int(sp.min()) < -1 or int(sp.max()) >= _ID_END):
        raise _bad_id()
    sp = sp.astype(np.int64)
    valid = sp >= 0
    ids, inv = np.unique(sp[valid], return_inverse=True)
    inv = inv.reshape(-1)
    seg_of = np.full(n, -1, np.int32)
    seg_of[valid] = inv
    order = np.flatnonzero(valid)[np.argsort(inv, kind='stable')].astype(np.int32)
    count = np.bincount(inv, minlength=ids.size)
    seg_start = np.zeros(ids.size + 1, np.int32)
    np.cumsum(count, out=seg_start[1:])
    return SuperpointIndex(n, ids.size, order.size, int(count.max()) if ids.size else 0, order, seg_of, seg_start)


def _rows(bits, n_points):
    """the bytes of packed rows: integer [n, ceil(N / 32)] words, or uint8 [n, >= ceil(N / 8)]"""
    bits = np.ascontiguousarray(_host(bits))
    if bits.ndim != 2 or bits.dtype.kind not in 'iu':
        raise ValueError(f'bits: integer rows [n, {(n_points + 31) // 32}] of 32-bit words')
    n = bits.shape[0]
    rows = bits.view(np.uint8).reshape(n, -1) if n else np.zeros((0, (n_points + 31) // 32 * 4), np.uint8)
    if n and rows.shape[1] * 8 < n_points:
        raise ValueError(f'bits: rows of {rows.shape[1] * 8} bits for {n_points} points')
    return rows


def _index_for(index, n_points):
    if not isinstance(index, SuperpointIndex):
        raise ValueError('index: a SuperpointIndex (superpoint_index(sp))')
    if index.n_points != n_points:
        raise ValueError(f'index: of {index.n_points} points, for {n_points}')
    return index


def mask_snap_numpy(bits, n_points, index, thr=0.5, mode='snap'):
    """The definition, on the host -> (out_bits int32 [n, ceil(N / 32)], npoint int32 [n])"""
    thr, mode = _thr_mode(thr, mode)
    n_points = int(n_points)
    idx = _index_for(index, n_points).numpy()
    rows = _rows(bits, n_points)
    n, words = rows.shape[0], (n_points + 31) // 32
    if n == 0 or n_points == 0:
        return np.zeros((n, words), np.int32), np.zeros(n, np.int32)
    dense = np.unpackbits(rows, axis=1, bitorder='little')[:, :n_points].astype(bool)
    out = dense.copy()
    if idx.n_seg:
        order, seg = idx.order.astype(np.intp), idx.seg_of.astype(np.intp)
        starts = idx.seg_start[:-1].astype(np.intp)
        size = np.diff(idx.seg_start.astype(np.int64))
        some = seg >= 0
        seg_some = seg[some]
        for k in range(n):
            inter = np.add.reduceat(dense[k, order].astype(np.int64), starts)
            taken = (inter >= 1) & (inter.astype(np.float64) / size.astype(np.float64) > thr)
            t = taken[seg_some]
            if mode == 'snap':
                out[k, some] = t
            elif mode == 'grow':
                out[k, some] |= t
            else:
                out[k, some] &= t
    pad = np.zeros((n, words * 32), bool)
    pad[:, :n_points] = out
    packed = np.ascontiguousarray(np.packbits(pad, axis=1, bitorder='little'))
    return packed.view(np.int32).reshape(n, words), out.sum(1).astype(np.int32)


def superpoint_vote_numpy(labels, index, n_classes, ignore_label=-100):
    """The definition, on the host -> labels after the vote, the dtype of ``labels``"""
    n_classes = _classes(n_classes)
    labels = _host(labels)
    if labels.ndim != 1 or labels.dtype.kind not in 'iu':
        raise ValueError('labels: a 1-D integer array, one label per point')
    idx = _index_for(index, labels.size).numpy()
    out = labels.copy()
    seg = idx.seg_of.astype(np.int64)
    lab = labels.astype(np.int64)
    counted = (seg >= 0) & (lab >= 0) & (lab < n_classes) & (lab != int(ignore_label))
    if counted.any():
        key, count = np.unique(seg[counted] * n_classes + lab[counted], return_counts=True)
        s, c = key // n_classes, key % n_classes
        first = np.lexsort((c, -count, s))                  # per segment: the greatest count, then the lowest class
        s, c = s[first], c[first]
        head = np.ones(s.size, bool)
        head[1:] = s[1:] != s[:-1]
        winner = np.full(idx.n_seg, -1, np.int64)
        winner[s[head]] = c[head]
        w = winner[np.maximum(seg, 0)]
        change = (seg >= 0) & (w >= 0)
        out[change] = w[change].astype(labels.dtype)
    return out


# ---- the device ------------------------------------------------------------------------------------------------------
def _index_device(sp):
    import torch

    from .. import _lib as L
    if sp.dim() != 1 or sp.is_floating_point() or sp.is_complex() or sp.dtype == torch.bool:
        raise ValueError('superpoint ids: a 1-D integer array, one id per point')
    dev = sp.device
    sp = sp.detach()
    if sp.dtype != torch.int32:
        # (an id outside the range stays outside it; narrower types cannot hold one above it)
        sp = (sp.clamp(-2, _ID_END) if sp.element_size() > 4 else sp).to(torch.int32)
    sp = sp.contiguous()
    n = sp.numel()
    lib = L.lib()
    with torch.cuda.device(dev):
        nb = lib.sg_superpoint_index_workspace_bytes(n)
        if nb == 0:
            raise L.SoftGroupHipError(f'superpoint_index: {n} points: outside the supported range (fewer than 2**31)')
        order = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        seg_of = torch.empty(n, dtype=torch.int32, device=dev)
        seg_start = torch.empty(n + 1, dtype=torch.int32, device=dev)
        meta = torch.empty(4, dtype=torch.int32, device=dev)
        ws = L.workspace(nb, dev)
        L.check(lib.sg_superpoint_index(L.ptr(sp) if n else None, n, L.ptr(order), L.ptr(seg_of) if n else None,
                                        L.ptr(seg_start), L.ptr(meta), L.ptr(ws), ws.numel(), L.stream()),
                'sg_superpoint_index')
        n_seg, flags, n_valid, max_size = meta.cpu().tolist()
    if flags:
        raise _bad_id()
    return SuperpointIndex(n, n_seg, n_valid, max_size, order[:n_valid], seg_of, seg_start[:n_seg + 1])


def superpoint_index(sp):
    """The segments of a cloud from its superpoint ids -> SuperpointIndex.  A CUDA tensor takes
    ``sg_superpoint_index`` (device arrays; one read-back, of ``meta``: the only one of the whole feature); numpy
    arrays and CPU tensors take ``superpoint_index_numpy``."""
    import torch
    if torch.is_tensor(sp) and sp.is_cuda:
        return _index_device(sp)
    return superpoint_index_numpy(sp)


def snap_device_raw(bits_ptr, n, n_points, index, thr, mode, device):
    """``sg_mask_snap`` on rows at a raw device address -> (out_bits int32 [n, words], npoint int32 [n]) on
    ``device``.  Nothing synchronises."""
    import torch

    from .. import _lib as L
    thr, mode = _thr_mode(thr, mode)
    n, n_points = int(n), int(n_points)
    idx = _index_for(index, n_points).cuda(device)
    words = (n_points + 31) // 32
    lib = L.lib()
    with torch.cuda.device(device):
        nb = lib.sg_mask_snap_workspace_bytes(n, n_points, idx.n_seg)
        if nb == 0:
            raise L.SoftGroupHipError(f'mask_snap: {n} masks over {n_points} points: outside the supported range '
                                      f'(at most {MAX_INSTANCES} masks, fewer than 2**31 points)')
        out_bits = torch.empty((n, words), dtype=torch.int32, device=device)
        npoint = torch.empty(n, dtype=torch.int32, device=device)
        ws = L.workspace(nb, device)
        some = idx.n_seg > 0
        L.check(lib.sg_mask_snap(bits_ptr, n, n_points, L.ptr(idx.order) if some else None,
                                 L.ptr(idx.seg_of) if n_points else None, L.ptr(idx.seg_start) if some else None,
                                 idx.n_seg, idx.n_valid, thr, _MODE[mode],
                                 L.ptr(out_bits) if out_bits.numel() else None, L.ptr(npoint) if n else None, L.ptr(ws), ws.numel(), L.stream()), 'sg_mask_snap')
    return out_bits, npoint


def mask_snap(bits, n_points, index, thr=0.5, mode='snap'):
    """-> (out_bits int32 [n, ceil(N / 32)], npoint int32 [n]) where ``bits`` lives.  CUDA bits: ``sg_mask_snap``
    (the index is brought to that device), no read-back.  CPU tensors and numpy arrays: ``mask_snap_numpy`` (tensors
    in, tensors out)."""
    import torch
    thr, mode = _thr_mode(thr, mode)
    n_points = int(n_points)
    words = (n_points + 31) // 32
    if not torch.is_tensor(bits):
        return mask_snap_numpy(bits, n_points, index, thr, mode)
    if bits.dim() != 2 or bits.element_size() != 4 or bits.is_floating_point() or bits.size(1) != words:
        raise ValueError(f'bits: an integer tensor [n, {words}] of 32-bit words')
    if not bits.is_cuda:
        out = mask_snap_numpy(bits.contiguous().numpy(), n_points, index, thr, mode)
        return tuple(torch.from_numpy(o) for o in out)
    bits = bits.contiguous()
    return snap_device_raw(bits.data_ptr() if bits.numel() else None, bits.size(0), n_points, index, thr, mode,
                           bits.device)


def _vote_device(labels, index, n_classes, ignore_label):
    import torch

    from .. import _lib as L
    if labels.dim() != 1 or labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool:
        raise ValueError('labels: a 1-D integer array, one label per point')
    dev = labels.device
    n = labels.numel()
    idx = _index_for(index, n).cuda(dev)
    if n_classes > MAX_CLASSES:
        raise L.SoftGroupHipError(f'superpoint_vote: {n_classes} classes, at most {MAX_CLASSES} on the device')
    labels = labels.detach().contiguous()
    lab32 = labels
    if labels.dtype != torch.int32:                         # (only 64-bit labels can lie outside 32 bits)
        lab32 = (labels.clamp(-2**31, 2**31 - 1) if labels.element_size() > 4 else labels).to(torch.int32)
    ignore = int(ignore_label) if 0 <= int(ignore_label) < n_classes else -1
    lib = L.lib()
    with torch.cuda.device(dev):
        nb = lib.sg_superpoint_vote_workspace_bytes(n, idx.n_seg, n_classes)
        if nb == 0:
            raise L.SoftGroupHipError(f'superpoint_vote: {n} points: outside the supported range (fewer than 2**31)')
        out = torch.empty(n, dtype=torch.int32, device=dev)
        ws = L.workspace(nb, dev)
        some = idx.n_seg > 0
        L.check(lib.sg_superpoint_vote(L.ptr(lab32) if n else None, n, L.ptr(idx.order) if some else None,
                                       L.ptr(idx.seg_of) if n else None, L.ptr(idx.seg_start), idx.n_seg, n_classes,
                                       ignore, L.ptr(out) if n else None, None, L.ptr(ws), ws.numel(), L.stream()),
                'sg_superpoint_vote')
        if labels.dtype != torch.int32:
            # a label the kernel left alone stays what it was, whatever the narrower words made of it
            out = torch.where(out == lab32, labels, out.to(labels.dtype))
    return out


def superpoint_vote(labels, index, n_classes, ignore_label=-100):
    """-> the labels after the vote, with the dtype and the location of ``labels``.  CUDA labels:
    ``sg_superpoint_vote`` (at most 256 classes, else ``SoftGroupHipError``), no read-back.  CPU tensors and numpy
    arrays: ``superpoint_vote_numpy``."""
    import torch
    n_classes = _classes(n_classes)
    if torch.is_tensor(labels) and labels.is_cuda:
        return _vote_device(labels, index, n_classes, ignore_label)
    out = superpoint_vote_numpy(labels, index, n_classes, ignore_label)
    return torch.from_numpy(out) if torch.is_tensor(labels) else out
