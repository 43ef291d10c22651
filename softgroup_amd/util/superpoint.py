"""Results refined on an over-segmentation ("superpoints"): instance masks snapped to whole superpoints and semantic
labels voted per superpoint, what nearly every ScanNet / S3DIS pipeline applies after the network (ScanNet ships
``*_vh_clean_2.0.010000.segs.json`` with every scene; ``voxel_downsample(xyz, 0.1)[1]`` is a valid superpoint id where
a dataset ships none).  The reference has no counterpart; the rules are those of ``softgroup_amd.ops.superpoint``:
a superpoint is taken by a mask when ``inter >= 1`` and ``inter / size > thr`` (strict, IEEE double); ``'snap'``
replaces the mask by its taken superpoints, ``'grow'`` only adds them, ``'trim'`` only removes the others; points in
no superpoint (id -1) keep what they had.

``superpoints`` is a ``SuperpointIndex`` (``ops.superpoint_index``) or the id array itself, which is indexed on the
spot -- on the device when it is a CUDA tensor or the device backend runs, so a CUDA id array never visits the host.

backends
  'numpy'   packed rows, ``mask_snap_numpy`` / ``superpoint_vote_numpy``, runs by ``np.diff`` on the host
  'device'  RLE text -> ``sg_inst_rle_parse`` -> ``sg_mask_bits_from_runs`` (the route of ``util/masks.py``; dense
            masks are packed on the host and uploaded) -> ``sg_mask_snap`` -> ``sg_mask_runs_count`` / ``_fill`` ->
            ``sg_rle_format_device`` -> ``rle_text_to_dicts``; labels through ``sg_superpoint_vote``.  RLE strings
            whose runs are not ascending raise, as in ``nms_instances``; so do more than 256 classes
  'auto'    numpy without a GPU; with one, what ``ops.superpoint._AUTO`` says per operation; strings whose runs are
            not ascending, a mask set beyond the device's run numbers and more than 256 classes take numpy.
            Both backends produce the same strings and labels byte for byte.
"""
import json

import numpy as np

from ..ops import resample as RS
from ..ops import superpoint as SP
from . import masks as M
from .lazy import LazyResults

__all__ = ['snap_instances', 'refine_result', 'load_scannet_segs']


def load_scannet_segs(path):
    """the ``segIndices`` of a ScanNet ``*.segs.json`` -> int32 [N], one superpoint id per vertex (host only)"""
    with open(path) as f:
        seg = np.asarray(json.load(f)['segIndices'])
    if seg.ndim != 1 or (seg.size and seg.dtype.kind not in 'iu'):
        raise ValueError(f'{path}: segIndices must be a flat list of integers')
    if seg.size and (seg.min() < -2**31 or seg.max() >= 2**31):
        raise ValueError(f'{path}: a segment id outside 32 bits')
    return seg.astype(np.int32)


class _Segments:
    """``superpoints`` as given, and ONE index built from it when the first step asks: the other location is a copy
    of that index, not a second build"""

    def __init__(self, superpoints):
        self._index = superpoints if isinstance(superpoints, SP.SuperpointIndex) else None
        self._ids = None if self._index is not None else superpoints
        self._host = self._dev = None

    def host(self):
        if self._host is None:
            if self._index is None:
                self._index = SP.superpoint_index_numpy(self._ids)
            self._host = self._index.numpy()
        return self._host

    def device(self, dev):
        import torch
        if self._dev is None:
            if self._index is None:
                ids = self._ids
                if not torch.is_tensor(ids):
                    ids = np.asarray(ids)
                    if ids.ndim != 1 or ids.dtype.kind not in 'iu':
                        raise ValueError('superpoint ids: a 1-D integer array, one id per point')
                    if ids.dtype == np.uint64:
                        ids = np.minimum(ids, np.uint64(2**63 - 1))     # (still outside the range of an id)
                    wide = ids.dtype.itemsize > 4 or ids.dtype == np.uint32
                    ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64 if wide else np.int32))
                self._index = SP.superpoint_index(ids if ids.is_cuda else ids.to(dev))
            self._dev = self._index.cuda(dev)
        return self._dev


def _segments(superpoints):
    return superpoints if isinstance(superpoints, _Segments) else _Segments(superpoints)


def _min_npoint(min_npoint):
    if int(min_npoint) != min_npoint or int(min_npoint) < 0:
        raise ValueError(f'min_npoint {min_npoint!r}: an integer >= 0')
    return int(min_npoint)


def _outputs(insts, keep, bits_host, n_points):
    """new dicts of the kept instances from their rows on the host: RLE in gives RLE out, a dense mask in gives a
    bool array out"""
    rows = bits_host.view(np.uint8)
    rle = [None] * len(keep)
    if any(isinstance(insts[s]['pred_mask'], dict) for s in keep):
        rle = M.rle_dicts_from_bits_numpy(bits_host, n_points)
    return [M.carried(insts[s], rle[g] if isinstance(insts[s]['pred_mask'], dict) else
                      np.unpackbits(rows[g], bitorder='little')[:n_points].astype(bool))
            for g, s in enumerate(keep)]


def _snap_numpy(insts, n_points, seg, thr, mode, min_npoint):
    out_bits, npoint = SP.mask_snap_numpy(M.packed_rows(insts, n_points), n_points, seg.host(), thr, mode)
    keep = np.flatnonzero(npoint >= min_npoint).tolist()
    return _outputs(insts, keep, np.ascontiguousarray(out_bits[keep]), n_points)


def _snap_device(insts, n_points, seg, thr, mode, min_npoint):
    import torch
    dev = torch.device('cuda', torch.cuda.current_device())
    n = len(insts)
    all_rle = all(isinstance(inst['pred_mask'], dict) for inst in insts)
    bits = M.checked_rows_device(insts, n_points, dev)
    out_bits, npoint = SP.snap_device_raw(bits.data_ptr() if bits.numel() else None, n, n_points, seg.device(dev), thr,
                                          mode, dev)
    keep = list(range(n))
    if min_npoint > 0:
        keep = torch.nonzero(npoint >= min_npoint).reshape(-1)
        out_bits = out_bits[keep].contiguous()
        keep = keep.cpu().tolist()
    if not keep:
        return []
    if not all_rle:
        return _outputs(insts, keep, out_bits.cpu().numpy(), n_points)
    masks = M.rle_dicts_from_bits_device(out_bits, n_points, dev)
    return [M.carried(insts[s], m) for s, m in zip(keep, masks)]


def snap_instances(pred_instances, superpoints, thr=0.5, mode='snap', min_npoint=0, backend='auto'):
    """The instances of ONE scan with every mask snapped to the superpoints (see the module text).
    ``pred_instances``: dicts of ``label_id``, ``conf`` and ``pred_mask`` (RLE dict as ``forward_test`` returns, or a
    dense array as ``load_pred_instances`` returns); ``superpoints``: a ``SuperpointIndex`` or the id array [N].
    -> NEW dicts in the input order with the source's ``scan_id``, ``label_id`` and ``conf`` and a ``pred_mask`` in
    the canonical RLE form (maximal runs, 1-based starts: ``rle_encode`` of the dense result) for an RLE source, a
    bool array for a dense one.  Instances whose snapped mask has fewer than ``min_npoint`` points are dropped.  The
    input list and its dicts are not modified."""
    thr, mode = SP._thr_mode(thr, mode)
    min_npoint = _min_npoint(min_npoint)
    chosen = SP.auto_backend(backend, 'snap')
    insts = list(pred_instances)
    if not insts:
        return []
    n_points = M.mask_length(insts)
    if chosen == 'device' and backend == 'auto' and not RS.mask_runs_supported(len(insts), n_points):
        chosen = 'numpy'                                    # (more runs than the device's int32 run numbers hold)
    return M.with_fallback(backend, chosen, _snap_device, _snap_numpy, insts, n_points, _segments(superpoints), thr,
                           mode, min_npoint)


def _vote(labels, seg, n_classes, ignore_label, backend):
    import torch
    chosen = SP.auto_backend(backend, 'vote')
    on_device = torch.is_tensor(labels) and labels.is_cuda
    if n_classes is None:
        n_classes = max(int(labels.max()) + 1, 1) if labels.shape[0] else 1
    n_classes = SP._classes(n_classes)
    if chosen == 'device' and backend == 'auto' and n_classes > SP.MAX_CLASSES:
        chosen = 'numpy'
    if chosen == 'device':
        dev = labels.device if on_device else torch.device('cuda', torch.cuda.current_device())
        d_labels = labels if on_device else torch.as_tensor(np.ascontiguousarray(SP._host(labels))).to(dev)
        out = SP.superpoint_vote(d_labels, seg.device(dev), n_classes, ignore_label)
        if on_device:
            return out
        return out.cpu() if torch.is_tensor(labels) else out.cpu().numpy()
    out = SP.superpoint_vote_numpy(labels, seg.host(), n_classes, ignore_label)
    if torch.is_tensor(labels):
        return torch.from_numpy(out).to(labels.device)
    return out


def refine_result(result, superpoints, masks=dict(thr=0.5, mode='snap', min_npoint=0), semantic=True, n_classes=None,
                  ignore_label=-100, backend='auto'):
    """-> a NEW result dict refined on the superpoints (see the module text).  ``result``: one result dict of
    ``forward_test`` / ``ScanForward`` (lazy results are resolved first); ``superpoints``: a ``SuperpointIndex`` or
    the id array [N]; one index serves both steps.

    * ``semantic_preds`` is voted per superpoint when ``semantic`` is true: ``n_classes`` defaults to
      ``max label + 1``; labels outside ``0 .. n_classes - 1`` (``ignore_label`` too) are not counted; the array keeps
      its dtype and its location;
    * ``pred_instances`` is snapped when ``masks`` is not None: ``masks`` holds ``thr``, ``mode`` and ``min_npoint``
      of ``snap_instances``;
    * EVERY OTHER KEY is passed through untouched, the same object: ``panoptic_preds`` and ``offset_preds`` are NOT
      recomputed from the refined masks and labels (and ``semantic_scores`` is not averaged)."""
    if isinstance(result, LazyResults):
        result.resolve()
    if masks is not None:
        extra = set(masks) - {'thr', 'mode', 'min_npoint'}
        if extra:
            raise ValueError(f'masks: unknown keys {sorted(extra)} (thr, mode, min_npoint)')
    seg = _segments(superpoints)
    out = {}
    for key, value in dict.items(result):
        if key == 'semantic_preds' and semantic:
            out[key] = _vote(value, seg, n_classes, ignore_label, backend)
        elif key == 'pred_instances' and masks is not None:
            out[key] = snap_instances(value, seg, masks.get('thr', 0.5), masks.get('mode', 'snap'),
                                      masks.get('min_npoint', 0), backend)
        else:
            out[key] = value
    return out
