"""De-duplicated instance lists: greedy mask NMS over what ``SoftGroup.get_instances`` / ``load_pred_instances``
return.  The reference has no counterpart (it hands every (proposal, class) pair to the evaluators); the rules
are those of ``softgroup_amd.ops.mask_nms``: descending ``conf``, the LOWER index first among equal scores, a
kept mask suppresses the later masks of its class whose ``inter / den`` exceeds ``thr``.

backends
  'numpy'   packed uint8 rows and popcounts on the host
  'device'  RLE text -> ``sg_inst_rle_parse`` -> ``sg_mask_bits_from_runs`` -> ``sg_mask_nms`` (dense masks are
            packed on the host and uploaded); one read-back of the keep flags
  'auto'    numpy without a GPU; with one, what ``_AUTO`` says: the device, which tools/mask_nms_bench.py
            measured ahead on every list (profiles/mask_nms_bench.txt, README); RLE strings whose runs are not
            ascending take numpy, which sorts them
"""
import numpy as np

from ..ops import nms as MN
from .results import _runs_of

__all__ = ['nms_instances']

# what 'auto' means with a GPU present (profiles/mask_nms_bench.txt: 0.4 - 1.4 ms against 9.6 - 878 ms)
_AUTO = 'device'


class _UnsortedRuns(ValueError):
    pass


def _choose(backend):
    if backend not in ('auto', 'device', 'numpy'):
        raise ValueError(f"backend {backend!r}: one of 'auto', 'device', 'numpy'")
    if backend == 'auto':
        import torch
        backend = _AUTO if torch.cuda.is_available() else 'numpy'
    return backend


def _length(insts):
    n_points = None
    for inst in insts:
        m = inst['pred_mask']
        k = int(m['length']) if isinstance(m, dict) else int(np.asarray(m).size)
        if n_points is None:
            n_points = k
        elif k != n_points:
            raise ValueError(f'masks of {n_points} and of {k} points in one list')
    return n_points


def _packed_row(mask, n_points, width):
    """packed uint8 row of one mask (RLE dict or dense array)"""
    if isinstance(mask, dict):
        _, starts, ends = _runs_of(mask)
        step = np.zeros(n_points + 1, dtype=np.uint8)       # +1 at a start, -1 (mod 256) at an end
        step[starts] = 1
        step[ends] = 255
        dense = np.cumsum(step[:-1], dtype=np.uint8)
    else:
        dense = np.asarray(mask).reshape(-1) != 0
    row = np.zeros(width, dtype=np.uint8)
    p = np.packbits(dense, bitorder='little')
    row[:p.size] = p
    return row


def _packed(insts, n_points):
    width = (n_points + 31) // 32 * 4
    rows = np.empty((len(insts), width), dtype=np.uint8)
    for k, inst in enumerate(insts):
        rows[k] = _packed_row(inst['pred_mask'], n_points, width)
    return rows


def _keep_numpy(insts, n_points, scores, labels, thr, measure, class_agnostic):
    return MN.mask_nms_numpy(_packed(insts, n_points), n_points, scores, labels, thr, measure, class_agnostic)[0]


def _bits_from_rle_device(insts, n_points, dev):
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
    return bits, flags, unsorted


def _keep_device(insts, n_points, scores, labels, thr, measure, class_agnostic):
    import torch
    dev = torch.device('cuda', torch.cuda.current_device())
    n = len(insts)
    check = None
    if all(isinstance(inst['pred_mask'], dict) for inst in insts):
        bits, flags, unsorted = _bits_from_rle_device(insts, n_points, dev)
        check = torch.stack([flags[0] != 0, unsorted])
    else:
        bits = torch.from_numpy(_packed(insts, n_points).view(np.int32)).to(dev)
    keep, _ = MN.mask_nms(bits, n_points, torch.from_numpy(scores).to(dev), torch.from_numpy(labels).to(dev),
                          thr, measure, class_agnostic)
    if check is not None:
        bad_text, bad_order = check.cpu().tolist()
        if bad_text:
            raise ValueError('malformed RLE text (a bad character, an odd token count or a run outside the mask)')
        if bad_order:
            raise _UnsortedRuns("RLE runs that are not ascending and disjoint: use backend='numpy'")
    assert keep.numel() == n
    return keep.cpu().numpy()


def nms_instances(pred_instances, thr=0.5, measure='iou', class_agnostic=False, backend='auto'):
    """The instances of ONE scan that survive greedy mask NMS: the same dict objects, in the same order.
    ``pred_instances``: dicts of ``label_id``, ``conf`` and ``pred_mask`` (RLE dict, or a dense array as
    ``load_pred_instances`` returns)."""
    MN._measure(measure)
    chosen = _choose(backend)
    insts = list(pred_instances)
    if not insts:
        return []
    n_points = _length(insts)
    scores = np.array([float(inst['conf']) for inst in insts], dtype=np.float32)
    labels = np.array([int(inst['label_id']) for inst in insts], dtype=np.int64).astype(np.int32)
    if not np.isfinite(scores).all():
        raise ValueError('nms_instances: scores must be finite')
    args = (insts, n_points, scores, labels, float(thr), measure, class_agnostic)
    if chosen == 'device':
        try:
            keep = _keep_device(*args)
        except _UnsortedRuns:
            if backend != 'auto':
                raise
            keep = _keep_numpy(*args)
    else:
        keep = _keep_numpy(*args)
    return [inst for inst, k in zip(insts, keep) if k]
