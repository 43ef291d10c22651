"""The mask-list codec: a list of instance dicts <-> packed bit rows <-> canonical RLE dicts, for the stages that work
on what ``SoftGroup.get_instances`` / ``load_pred_instances`` return (``nms_instances``, ``split_instances``,
``snap_instances``, ``propagate_result``, ``stitch_results``).  A ``pred_mask`` is an RLE dict or a dense array.

list in
  host     ``packed_rows``: uint8 rows of 32-bit words, little-endian bit order; an RLE string paints what
           ``rle_decode`` paints, whatever order its runs are in
  device   ``rows_device``: the strings laid end to end -> ``sg_inst_rle_parse`` -> ``sg_mask_bits_from_runs``; a list
           with a dense mask is packed on the host and uploaded.  The expansion needs ascending, disjoint runs inside
           a mask (what the encoders here write): ``check`` holds the two flags [malformed text, unsorted runs] ON THE
           DEVICE, so that a caller can fold them into a read-back it makes anyway; ``checked_rows_device`` reads them
           back on the spot; ``raise_bad_rle`` turns them into the two errors
list out
  ``rle_dicts_from_bits_*`` / ``rle_dicts_from_runs_*``: maximal runs, 1-based starts -- ``rle_encode`` of the dense
  mask byte for byte; on the device through ``sg_rle_format_device`` and one read-back of the text offsets
"""
import numpy as np

from ..ops import nms as MN
from ..ops import resample as RS
from .results import _runs_of
from .rle import rle_encode_runs, rle_text_to_dicts

_CARRIED = ('scan_id', 'label_id', 'conf')
# what a result over the full cloud takes from ``gt`` and never from the scans of its parts
_FROM_GT = ('semantic_labels', 'instance_labels', 'offset_labels', 'color_feats', 'gt_instances')


class UnsortedRuns(ValueError):
    pass


def carried(inst, pred_mask):
    """a new dict with the ``scan_id``, ``label_id`` and ``conf`` of ``inst`` (those it has) and ``pred_mask``"""
    return dict({k: inst[k] for k in _CARRIED if k in inst}, pred_mask=pred_mask)


def with_fallback(backend, chosen, device_fn, numpy_fn, *args):
    """the device half, and the numpy half where 'auto' meets RLE strings whose runs are not ascending"""
    if chosen == 'device':
        try:
            return device_fn(*args)
        except UnsortedRuns:
            if backend != 'auto':
                raise
    return numpy_fn(*args)


def full_cloud_coords(coords, n_points, of):
    if int(coords.shape[0]) != n_points:
        raise ValueError(f'coords: {coords.shape[0]} points for {of} of {n_points}')
    return coords


def take_from_gt(out, gt):
    for key in _FROM_GT:
        if key in gt:
            out[key] = gt[key]


# ---- list in ---------------------------------------------------------------------------------------------------------
def mask_length(insts):
    n_points = None
    for inst in insts:
        m = inst['pred_mask']
        k = int(m['length']) if isinstance(m, dict) else int(np.asarray(m).size)
        if n_points is None:
            n_points = k
        elif k != n_points:
            raise ValueError(f'masks of {n_points} and of {k} points in one list')
    return n_points


def dense_of(mask, n_points):
    """uint8 [n_points] of zeros and ones: one mask (RLE dict or dense array)"""
    if isinstance(mask, dict):
        _, starts, ends = _runs_of(mask)
        step = np.zeros(n_points + 1, dtype=np.uint8)       # +1 at a start, -1 (mod 256) at an end
        step[starts] = 1
        step[ends] = 255
        return np.cumsum(step[:-1], dtype=np.uint8)
    return (np.asarray(mask).reshape(-1) != 0).view(np.uint8)


def packed_rows(insts, n_points):
    """uint8 [n, ceil(n_points / 32) * 4]: the packed rows of a list"""
    rows = np.zeros((len(insts), (n_points + 31) // 32 * 4), dtype=np.uint8)
    for k, inst in enumerate(insts):
        p = np.packbits(dense_of(inst['pred_mask'], n_points), bitorder='little')
        rows[k, :p.size] = p
    return rows


def _rows_from_rle_device(insts, n_points, dev):
    """bit rows of RLE dicts: the strings laid end to end, parsed and expanded on the device"""
    import torch

    from .. import _lib as L
    lib = L.lib()
    texts = [inst['pred_mask']['counts'] for inst in insts]
    try:
        text = ''.join(texts).encode('ascii')
    except UnicodeEncodeError:
        raise ValueError('malformed RLE text: a character that is neither a digit nor white space')
    n, n_text = len(texts), len(text)
    text_off = np.zeros(n + 1, np.int64)
    text_off[1:] = np.cumsum(np.array([len(t) for t in texts], np.int64))
    slots = int(lib.sg_inst_rle_run_slots(n_text, n))
    bounds = (text_off + np.arange(n + 1)) // 4             # mask m's slots start at (text_off[m] + m) / 4
    bounds[n] = slots                                       # the last mask owns the spare slots
    d_text = torch.from_numpy(np.frombuffer(text, np.uint8).copy() if n_text else np.zeros(1, np.uint8)).to(dev)
    d_off, d_bounds = torch.from_numpy(text_off).to(dev), torch.from_numpy(bounds).to(dev)
    runs = torch.empty((3, slots), dtype=torch.int32, device=dev)
    vert = torch.empty(n, dtype=torch.int32, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    L.check(lib.sg_inst_rle_parse(L.ptr(d_text), L.ptr(d_off), None, n, n_text, n_points, L.ptr(runs[0]),
                                  L.ptr(runs[1]), L.ptr(runs[2]), slots, L.ptr(vert), L.ptr(flags), L.stream()),
            'sg_inst_rle_parse')
    start, length, owner = runs[0], runs[1], runs[2]
    some = length > 0
    big = torch.iinfo(torch.int32).max                      # empty slots sort behind every run of their mask
    starts = torch.where(some, start, big)
    ends = torch.where(some, start + length, big)
    # the expansion needs ascending, disjoint runs inside a mask (what the encoders here write)
    same = owner[1:] == owner[:-1]
    unsorted = (same & some[1:] & (starts[1:] < ends[:-1])).any()
    bits = MN.mask_bits_from_runs(starts.contiguous(), ends.contiguous(), d_bounds, n_points)
    return bits, torch.stack([flags[0] != 0, unsorted])


def rows_device(insts, n_points, dev):
    """-> (bits int32 [n, ceil(n_points / 32)] on ``dev``, check): ``check`` is the device tensor of the two flags
    [bad_text, bad_order] for an all-RLE list, None for a list with a dense mask.  No read-back."""
    import torch
    if all(isinstance(inst['pred_mask'], dict) for inst in insts):
        return _rows_from_rle_device(insts, n_points, dev)
    return torch.from_numpy(packed_rows(insts, n_points).view(np.int32)).to(dev), None


def raise_bad_rle(bad_text, bad_order):
    if bad_text:
        raise ValueError('malformed RLE text (a bad character, an odd token count or a run outside the mask)')
    if bad_order:
        raise UnsortedRuns("RLE runs that are not ascending and disjoint: use backend='numpy'")


def checked_rows_device(insts, n_points, dev):
    """``rows_device`` with its check read back and raised: one small copy for an all-RLE list"""
    bits, check = rows_device(insts, n_points, dev)
    if check is not None:
        raise_bad_rle(*check.cpu().tolist())
    return bits


# ---- list out --------------------------------------------------------------------------------------------------------
def rle_dicts_from_runs_device(starts, ends, bounds, n, n_points, dev, extra=None):
    """Runs on the device (``starts`` / ``ends`` int32, ``bounds`` int64 [n + 1]) -> the n RLE dicts:
    ``sg_rle_format_device``, ONE read-back of the text offsets, the text.  ``extra``: a small integer tensor that
    travels with the offsets -> (dicts, its values)."""
    import torch

    from .. import _lib as L
    lib = L.lib()
    with torch.cuda.device(dev):
        cap = max(int(starts.numel()), 1)
        tcap = int(lib.sg_rle_format_device_text_bytes(cap, n_points))
        text = torch.empty(tcap, dtype=torch.uint8, device=dev)
        text_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        ws = L.workspace(lib.sg_rle_format_device_workspace_bytes(cap), dev)
        L.check(lib.sg_rle_format_device(L.ptr(starts), L.ptr(ends), L.ptr(bounds), n, cap, n_points, L.ptr(text), tcap,
                                         L.ptr(text_off), L.ptr(ws), ws.numel(), L.stream()), 'sg_rle_format_device')
        if extra is None:
            return rle_text_to_dicts(n_points, text, text_off.cpu().tolist())
        back = torch.cat([text_off, extra.long()]).cpu().tolist()
        return rle_text_to_dicts(n_points, text, back[:n + 1]), back[n + 1:]


def rle_dicts_from_bits_device(bits, n_points, dev):
    """CUDA bit rows -> RLE dicts: ``mask_runs_from_bits`` (one read-back, the run total) and the above"""
    starts, ends, bounds = RS.mask_runs_from_bits(bits, n_points)
    return rle_dicts_from_runs_device(starts, ends, bounds, bits.size(0), n_points, dev)


def rle_dicts_from_runs_numpy(starts, ends, bounds, n_points):
    """host runs (0-based, end exclusive, ``bounds`` [n + 1]) -> the n RLE dicts"""
    return [rle_encode_runs(n_points, starts[bounds[g]:bounds[g + 1]],
                            ends[bounds[g]:bounds[g + 1]] - starts[bounds[g]:bounds[g + 1]])
            for g in range(len(bounds) - 1)]


def rle_dicts_from_bits_numpy(bits, n_points):
    return rle_dicts_from_runs_numpy(*RS.mask_runs_from_bits_numpy(bits, n_points), n_points)
