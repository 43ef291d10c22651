"""De-duplicated instance lists: greedy mask NMS over what ``SoftGroup.get_instances`` / ``load_pred_instances``
return.  The reference has no counterpart (it hands every (proposal, class) pair to the evaluators); the rules
are those of ``softgroup_amd.ops.mask_nms``: descending ``conf``, the LOWER index first among equal scores, a
kept mask suppresses the later masks of its class whose ``inter / den`` exceeds ``thr``.

backends
  'numpy'   packed uint8 rows and popcounts on the host
  'device'  RLE text -> ``sg_inst_rle_parse`` -> ``sg_mask_bits_from_runs`` -> ``sg_mask_nms`` (dense masks are
            packed on the host and uploaded: ``util/masks.py``); one read-back of the keep flags
  'auto'    numpy without a GPU; with one, what ``_AUTO`` says: the device, which tools/mask_nms_bench.py
            measured ahead on every list (profiles/mask_nms_bench.txt, README); RLE strings whose runs are not
            ascending take numpy, which sorts them
"""
import numpy as np

from ..ops import nms as MN
from ..ops._args import choose_backend
from . import masks as M

__all__ = ['nms_instances']

# what 'auto' means with a GPU present (profiles/mask_nms_bench.txt: 0.4 - 1.4 ms against 9.6 - 878 ms)
_AUTO = 'device'


def _keep_numpy(insts, n_points, scores, labels, thr, measure, class_agnostic):
    return MN.mask_nms_numpy(M.packed_rows(insts, n_points), n_points, scores, labels, thr, measure, class_agnostic)[0]


def _keep_device(insts, n_points, scores, labels, thr, measure, class_agnostic):
    import torch
    dev = torch.device('cuda', torch.cuda.current_device())
    bits, check = M.rows_device(insts, n_points, dev)
    keep, _ = MN.mask_nms(bits, n_points, torch.from_numpy(scores).to(dev), torch.from_numpy(labels).to(dev),
                          thr, measure, class_agnostic)
    if check is not None:                                   # (read back with mask_nms already enqueued)
        M.raise_bad_rle(*check.cpu().tolist())
    assert keep.numel() == len(insts)
    return keep.cpu().numpy()


def nms_instances(pred_instances, thr=0.5, measure='iou', class_agnostic=False, backend='auto'):
    """The instances of ONE scan that survive greedy mask NMS: the same dict objects, in the same order.
    ``pred_instances``: dicts of ``label_id``, ``conf`` and ``pred_mask`` (RLE dict, or a dense array as
    ``load_pred_instances`` returns)."""
    MN._measure(measure)
    chosen = choose_backend(backend, _AUTO)
    insts = list(pred_instances)
    if not insts:
        return []
    n_points = M.mask_length(insts)
    scores = np.array([float(inst['conf']) for inst in insts], dtype=np.float32)
    labels = np.array([int(inst['label_id']) for inst in insts], dtype=np.int64).astype(np.int32)
    if not np.isfinite(scores).all():
        raise ValueError('nms_instances: scores must be finite')
    args = (insts, n_points, scores, labels, float(thr), measure, class_agnostic)
    keep = M.with_fallback(backend, chosen, _keep_device, _keep_numpy, *args)
    return [inst for inst, k in zip(insts, keep) if k]
