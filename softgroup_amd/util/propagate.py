"""A result of a THINNED cloud re-expressed over the full cloud the user owns: what follows a scan of
``xyz[sample_ids]`` (``softgroup_amd.data.voxel_downsample`` / ``random_downsample``) so that ``save_results``,
``save_visualizations``, ``evaluate_box_ap`` and the evaluators get one entry per original point.  The reference has
no counterpart.

``index`` [N_full] says which point of the result every original point takes its prediction from: the ``inverse``
of ``voxel_downsample``, or what ``softgroup_amd.ops.resample.nearest_index(thinned_xyz, full_xyz)`` returned
(-1 = none, e.g. beyond ``max_dist``).

rules
  * ``semantic_preds`` gathered, ``ignore_label`` where ``index < 0``; ``offset_preds`` and ``panoptic_preds``
    gathered, 0 there;
  * ``coords_float`` becomes ``coords`` when given and is dropped otherwise (the thinned coordinates are not the
    full cloud's);
  * ``semantic_labels``, ``instance_labels``, ``offset_labels`` (and ``color_feats``, ``gt_instances``) are taken
    from ``gt`` when it has them and dropped otherwise -- never gathered from the thinned scan;
  * ``pred_instances``: the same ``scan_id``, ``label_id`` and ``conf``; ``pred_mask`` an RLE dict of
    ``length = N_full`` in canonical form (maximal runs, 1-based starts); empty masks stay in the list;
  * every other key is copied.  The input dict and its instance dicts are not modified.

backends (the masks; the dense arrays are plain gathers where they live)
  'numpy'   decode, take, encode on the host
  'device'  RLE text -> ``sg_inst_rle_parse`` -> ``sg_mask_bits_from_runs`` (the route of ``util/masks.py``) ->
            ``sg_mask_bits_gather`` -> ``sg_mask_runs_count`` / ``_fill`` -> ``sg_rle_format_device`` ->
            ``rle_text_to_dicts``; RLE strings whose runs are not ascending raise, as in ``nms_instances``
  'auto'    numpy without a GPU; with one, what ``ops.resample._AUTO['masks']`` says; strings whose runs are not
            ascending take numpy, and so does a mask set beyond the device's range (``n_inst * ceil(N_full / 2)``
            at or above 2**31, e.g. 1000 masks over 5 M points), where ``'device'`` raises ``SoftGroupHipError``.
            Both backends produce the same strings byte for byte.

A CUDA ``index`` stays on the device for the device backend and for CUDA arrays of the result (one read-back of its
minimum and maximum for the range check); it is brought to the host only when a numpy array or the numpy backend
needs it.
"""
import numpy as np

from ..ops import resample as RS
from . import masks as M
from .lazy import LazyResults
from .rle import rle_encode_runs

__all__ = ['propagate_result']

_GATHERED = {'semantic_preds': None, 'offset_preds': 0, 'panoptic_preds': 0}      # key -> fill (None: ignore_label)


class _Index:
    """``index`` validated once, with a host and a device copy made only when something needs them: a CUDA
    ``inverse`` of ``voxel_downsample`` stays on the device for the device backend and CUDA arrays"""

    def __init__(self, index):
        import torch
        self._host = self._dev = None
        if torch.is_tensor(index):
            index = index.detach()
            if index.dim() != 1 or index.is_floating_point() or index.is_complex() or index.dtype == torch.bool:
                raise ValueError('index: a 1-D integer array, one entry per point of the full cloud')
            if index.is_cuda:
                self._dev = index.long().contiguous()
            else:
                self._host = np.ascontiguousarray(index.numpy(), dtype=np.int64)
        else:
            index = np.asarray(index)
            if index.ndim != 1 or index.dtype.kind not in 'iu':
                raise ValueError('index: a 1-D integer array, one entry per point of the full cloud')
            self._host = np.ascontiguousarray(index, dtype=np.int64)
        self.size = int(self._host.size if self._dev is None else self._dev.numel())

    def bounds(self):
        """(min, max) of a non-empty index -- one read-back when it lives on the device"""
        if self._host is not None:
            return int(self._host.min()), int(self._host.max())
        import torch
        return tuple(torch.stack([self._dev.min(), self._dev.max()]).cpu().tolist())

    def host(self):
        if self._host is None:
            self._host = self._dev.cpu().numpy()
        return self._host

    def device(self, dev):
        import torch
        if self._dev is None:
            self._dev = torch.from_numpy(self._host).to(dev)
        return self._dev.to(dev)                              # (a copy only for another card)


def _gather(arr, idx, fill):
    """arr[idx] along axis 0 with ``fill`` where idx < 0; numpy arrays stay numpy, tensors stay where they are"""
    import torch
    if torch.is_tensor(arr):
        t_idx = idx.device(arr.device) if arr.is_cuda else torch.from_numpy(idx.host())
        out = arr[t_idx.clamp(min=0)]
        out[t_idx < 0] = fill
        return out
    arr = np.asarray(arr)
    h_idx = idx.host()
    out = arr[np.maximum(h_idx, 0)]
    out[h_idx < 0] = fill
    return out


def _masks_numpy(insts, n_src, idx):
    idx = idx.host()
    n_full = idx.size
    ok = idx >= 0
    src_of = idx[ok]
    out = []
    for inst in insts:
        pad = np.zeros(n_full + 2, dtype=np.int8)
        pad[1:-1][ok] = M.dense_of(inst['pred_mask'], n_src)[src_of]
        edge = np.diff(pad)
        starts = np.flatnonzero(edge == 1)
        out.append(rle_encode_runs(n_full, starts, np.flatnonzero(edge == -1) - starts))
    return out


def _masks_device(insts, n_src, idx):
    import torch
    dev = torch.device('cuda', torch.cuda.current_device())
    bits = M.checked_rows_device(insts, n_src, dev)
    out = RS.mask_bits_gather(bits, n_src, idx.device(dev).to(torch.int32))
    return M.rle_dicts_from_bits_device(out, idx.size, dev)


def propagate_result(result, index, coords=None, gt=None, ignore_label=-100, backend='auto'):
    """-> a NEW result dict over the ``len(index)`` points of the full cloud (see the module text).
    ``result``: one result dict of ``forward_test`` / ``ScanForward`` on the thinned cloud (lazy results are
    resolved first, as ``save_results`` does); ``index``: int [N_full] into its points, -1 = none; ``coords``:
    the full cloud's coordinates [N_full, 3]; ``gt``: dict of the full cloud's label arrays."""
    chosen = RS.auto_backend(backend, 'masks')
    if isinstance(result, LazyResults):
        result.resolve()
    idx = _Index(index)
    n_full = idx.size
    insts = list(result['pred_instances']) if 'pred_instances' in result else None
    n_src = None
    for key in _GATHERED:
        if key in result:
            n_src = int(result[key].shape[0])
            break
    if n_src is None and insts:
        n_src = M.mask_length(insts)
    lo, hi = idx.bounds() if n_full else (0, -1)
    if n_src is None:
        n_src = hi + 1
    if hi >= n_src or lo < -1:
        raise ValueError(f'index: entries between -1 and {n_src - 1} (the result has {n_src} points)')
    gt = gt or {}
    out = {}
    for key, value in dict.items(result):
        if key in _GATHERED:
            if int(value.shape[0]) != n_src:
                raise ValueError(f'{key}: {value.shape[0]} entries in a result of {n_src} points')
            out[key] = _gather(value, idx, ignore_label if _GATHERED[key] is None else _GATHERED[key])
        elif key == 'coords_float':
            if coords is not None:
                out[key] = M.full_cloud_coords(coords, n_full, 'an index')
        elif key in M._FROM_GT or key == 'pred_instances':
            pass
        else:
            out[key] = value
    if coords is not None and 'coords_float' not in out:
        out['coords_float'] = coords
    M.take_from_gt(out, gt)
    if insts is not None:
        if insts and M.mask_length(insts) != n_src:
            raise ValueError(f'pred_instances: masks of {M.mask_length(insts)} points in a result of {n_src} points')
        masks = []
        if insts:
            if chosen == 'device' and backend == 'auto' and not RS.mask_runs_supported(len(insts), n_full):
                chosen = 'numpy'                         # (more runs than the device's int32 run numbers hold)
            masks = M.with_fallback(backend, chosen, _masks_device, _masks_numpy, insts, n_src, idx)
        out['pred_instances'] = [dict(inst, pred_mask=m) for inst, m in zip(insts, masks)]
    return out
