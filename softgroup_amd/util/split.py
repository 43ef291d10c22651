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
  'device'  RLE text -> ``sg_inst_rle_parse`` -> ``sg_mask_bits_from_runs`` (the route of ``util/masks.py``; dense
            masks are packed on the host and uploaded) -> ``sg_mask_split_count`` / ``_fill`` ->
            ``sg_mask_runs_count`` / ``_fill`` -> ``sg_rle_format_device`` -> ``rle_text_to_dicts``; RLE strings
            whose runs are not ascending raise, as in ``nms_instances``
  'auto'    numpy without a GPU; with one, what ``_AUTO`` says: the device, which tools/split_bench.py measured
            ahead on every list (profiles/split_bench.txt, README); RLE strings whose runs are not ascending take
            numpy, which sorts them.  Both backends produce the same strings byte for byte.
"""
import numpy as np

from ..ops import split as MS
from ..ops._args import choose_backend
from . import masks as M
from . import nms as UN

__all__ = ['split_instances', 'apply_split']

# what 'auto' means with a GPU present (profiles/split_bench.txt: 2.6 - 21 ms against 2.2 - 35 s)
_AUTO = 'device'


def _outputs(insts, source, masks):
    return [M.carried(insts[s], m) for s, m in zip(source, masks)]


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
    out_bits, source, _ = MS.mask_components_numpy(M.packed_rows(insts, n_points), n_points, coords, radius,
                                                   min_npoint, mode)
    if source.size == 0:
        return []
    return _outputs(insts, source.tolist(), M.rle_dicts_from_bits_numpy(out_bits, n_points))


def split_rows_device(bits_ptr, n, n_points, coords, insts, radius, min_npoint, mode, device):
    """The device path from bit rows at a raw address (a tensor's, or the rows a scan left in its arena) to the
    output list: components, runs, RLE text.  ``insts``: the n dicts the rows belong to."""
    import torch
    coords = torch.as_tensor(coords)
    out_bits, source, _ = MS.components_device_raw(bits_ptr, n, n_points, coords, radius, min_npoint, mode, device)
    if out_bits.size(0) == 0:
        return []
    masks = M.rle_dicts_from_bits_device(out_bits, n_points, device)
    return _outputs(insts, source.cpu().tolist(), masks)


def _split_device(insts, n_points, coords, radius, min_npoint, mode):
    import torch
    dev = torch.device('cuda', torch.cuda.current_device())
    bits = M.checked_rows_device(insts, n_points, dev)
    return split_rows_device(bits.data_ptr() if bits.numel() else None, len(insts), n_points, coords, insts, radius,
                             min_npoint, mode, dev)


def split_instances(pred_instances, coords, radius, min_npoint=1, mode='split', backend='auto'):
    """The instances of ONE scan with every mask cut into its connected components (see the module text).
    ``pred_instances``: dicts of ``label_id``, ``conf`` and ``pred_mask`` (RLE dict, or a dense array as
    ``load_pred_instances`` returns); ``coords``: the [N, 3] coordinates the masks index (numpy or tensor)."""
    radius, min_npoint, mode = MS._args(radius, min_npoint, mode)
    chosen = choose_backend(backend, _AUTO)
    insts = list(pred_instances)
    if not insts:
        return []
    n_points = M.mask_length(insts)
    coords = _coords(coords, n_points)
    return M.with_fallback(backend, chosen, _split_device, _split_numpy, insts, n_points, coords, radius, min_npoint,
                           mode)


def apply_split(pred_instances, coords, split, nms, backend='auto'):
    """What ``SoftGroup.forward_test`` and ``ScanForward`` do to their finished list: with ``test_cfg.split`` absent
    or None the list itself; else the split list and, when ``test_cfg.nms`` is set as well, ``nms_instances`` of
    that -- the stage that makes masks smaller runs before the one that compares them."""
    if split is None:
        return pred_instances
    radius, min_npoint, mode = MS.split_params(split)
    if pred_instances:
        assert int(coords.shape[0]) == M.mask_length(pred_instances), 'coords must be the points the masks index'
    out = split_instances(pred_instances, coords, radius, min_npoint, mode, backend)
    if nms is not None:
        from ..ops.nms import nms_params
        out = UN.nms_instances(out, *nms_params(nms), backend=backend)
    return out
