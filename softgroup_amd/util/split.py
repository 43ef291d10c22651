"""Instance lists whose masks are cut into their spatially connected components: what follows
``SoftGroup.get_instances`` / ``load_pred_instances`` when one predicted mask may be an object plus stray points
elsewhere, or two objects welded into one proposal.  The reference has no counterpart; the rules are those of
``softgroup_amd.ops.split.mask_components``: inside one mask two points are adjacent within ``radius`` (inclusive,
IEEE double), ``'split'`` keeps every component of at least ``min_npoint`` points, ``'largest'`` the greatest per
mask; outputs in ascending (source instance, smallest point) order.

Every output is a NEW dict with the ``scan_id``, ``label_id`` and ``conf`` of its source and a ``pred_mask`` in the
canonical RLE form (maximal runs, 1-based starts: ``rle_encode`` of the dense component, byte for byte).  The input
list and its dicts are not modified.

backends
  'numpy'   packed rows, ``mask_components_numpy``, runs by ``np.diff`` on the host
  'device'  RLE text -> ``sg_inst_rle_parse`` -> ``sg_mask_bits_from_runs`` (the route of ``util/nms.py``; dense
            masks are packed on the host and uploaded) -> ``sg_mask_split_count`` / ``_fill`` ->
            ``sg_mask_runs_count`` / ``_fill`` -> ``sg_rle_format_device`` -> ``rle_text_to_dicts``; RLE strings
            whose runs are not ascending raise, as in ``nms_instances``
  'auto'    numpy without a GPU; with one, what ``_AUTO`` says: the device, which tools/split_bench.py measured
            ahead on every list (profiles/split_bench.txt, README); RLE strings whose runs are not ascending take
            numpy, which sorts them.  Both backends produce the same strings byte for byte.
"""
import numpy as np

from ..ops import resample as RS
from ..ops import split as MS
from . import nms as UN
from .rle import rle_encode_runs, rle_text_to_dicts

__all__ = ['split_instances', 'apply_split']

# what 'auto' means with a GPU present (profiles/split_bench.txt: 2.6 - 21 ms against 2.2 - 35 s)
_AUTO = 'device'

_CARRIED = ('scan_id', 'label_id', 'conf')


def _choose(backend):
    if backend not in ('auto', 'device', 'numpy'):
        raise ValueError(f"backend {backend!r}: one of 'auto', 'device', 'numpy'")
    if backend == 'auto':
        import torch
        backend = _AUTO if torch.cuda.is_available() else 'numpy'
    return backend


def _outputs(insts, source, masks):
    return [dict({k: insts[s][k] for k in _CARRIED if k in insts[s]}, pred_mask=m) for s, m in zip(source, masks)]


def _coords(coords, n_points):
    import torch
    shape = tuple(coords.shape)
    if shape != (n_points, 3):
        raise ValueError(f'coords: {shape} for masks of {n_points} points: an array [{n_points}, 3]')
    return coords if torch.is_tensor(coords) else np.ascontiguousarray(coords, dtype=np.float32)


def _split_numpy(insts, n_points, coords, radius, min_npoint, mode):
    import torch
    if torch.is_tensor(coords):
        coords = coords.detach().cpu().numpy()
    out_bits, source, _ = MS.mask_components_numpy(UN._packed(insts, n_points), n_points, coords, radius, min_npoint,
                                                   mode)
    if source.size == 0:
        return []
    starts, ends, bounds = RS.mask_runs_from_bits_numpy(out_bits, n_points)
    masks = [rle_encode_runs(n_points, starts[bounds[g]:bounds[g + 1]],
                             ends[bounds[g]:bounds[g + 1]] - starts[bounds[g]:bounds[g + 1]])
             for g in range(source.size)]
    return _outputs(insts, source.tolist(), masks)


def split_rows_device(bits_ptr, n, n_points, coords, insts, radius, min_npoint, mode, device):
    """The device path from bit rows at a raw address (a tensor's, or the rows a scan left in its arena) to the
    output list: components, runs, RLE text.  ``insts``: the n dicts the rows belong to."""
    import torch

    from .. import _lib as L
    lib = L.lib()
    coords = torch.as_tensor(coords)
    out_bits, source, _ = MS.components_device_raw(bits_ptr, n, n_points, coords, radius, min_npoint, mode, device)
    n_out = out_bits.size(0)
    if n_out == 0:
        return []
    with torch.cuda.device(device):
        starts, ends, bounds = RS.mask_runs_from_bits(out_bits, n_points)
        cap = max(int(starts.numel()), 1)
        tcap = int(lib.sg_rle_format_device_text_bytes(cap, n_points))
        text = torch.empty(tcap, dtype=torch.uint8, device=device)
        text_off = torch.empty(n_out + 1, dtype=torch.int64, device=device)
        ws = L.workspace(lib.sg_rle_format_device_workspace_bytes(cap), device)
        L.check(lib.sg_rle_format_device(L.ptr(starts), L.ptr(ends), L.ptr(bounds), n_out, cap, n_points, L.ptr(text),
                                         tcap, L.ptr(text_off), L.ptr(ws), ws.numel(), L.stream()),
                'sg_rle_format_device')
        source = source.cpu().tolist()
        masks = rle_text_to_dicts(n_points, text, text_off.cpu().tolist())
    return _outputs(insts, source, masks)


def _split_device(insts, n_points, coords, radius, min_npoint, mode):
    import torch
    dev = torch.device('cuda', torch.cuda.current_device())
    if all(isinstance(inst['pred_mask'], dict) for inst in insts):
        bits, flags, unsorted = UN._bits_from_rle_device(insts, n_points, dev)
        bad_text, bad_order = torch.stack([flags[0] != 0, unsorted]).cpu().tolist()
        if bad_text:
            raise ValueError('malformed RLE text (a bad character, an odd token count or a run outside the mask)')
        if bad_order:
            raise UN._UnsortedRuns("RLE runs that are not ascending and disjoint: use backend='numpy'")
    else:
        bits = torch.from_numpy(UN._packed(insts, n_points).view(np.int32)).to(dev)
    return split_rows_device(bits.data_ptr() if bits.numel() else None, len(insts), n_points, coords, insts, radius,
                             min_npoint, mode, dev)


def split_instances(pred_instances, coords, radius, min_npoint=1, mode='split', backend='auto'):
    """The instances of ONE scan with every mask cut into its connected components (see the module text).
    ``pred_instances``: dicts of ``label_id``, ``conf`` and ``pred_mask`` (RLE dict, or a dense array as
    ``load_pred_instances`` returns); ``coords``: the [N, 3] coordinates the masks index (numpy or tensor)."""
    radius, min_npoint, mode = MS._args(radius, min_npoint, mode)
    chosen = _choose(backend)
    insts = list(pred_instances)
    if not insts:
        return []
    n_points = UN._length(insts)
    coords = _coords(coords, n_points)
    args = (insts, n_points, coords, radius, min_npoint, mode)
    if chosen == 'device':
        try:
            return _split_device(*args)
        except UN._UnsortedRuns:
            if backend != 'auto':
                raise
    return _split_numpy(*args)


def apply_split(pred_instances, coords, split, nms, backend='auto'):
    """What ``SoftGroup.forward_test`` and ``ScanForward`` do to their finished list: with ``test_cfg.split`` absent
    or None the list itself; else the split list and, when ``test_cfg.nms`` is set as well, ``nms_instances`` of
    that -- the stage that makes masks smaller runs before the one that compares them."""
    if split is None:
        return pred_instances
    radius, min_npoint, mode = MS.split_params(split)
    if pred_instances:
        assert int(coords.shape[0]) == UN._length(pred_instances), 'coords must be the points the masks index'
    out = split_instances(pred_instances, coords, radius, min_npoint, mode, backend)
    if nms is not None:
        from ..ops.nms import nms_params
        out = UN.nms_instances(out, *nms_params(nms), backend=backend)
    return out
