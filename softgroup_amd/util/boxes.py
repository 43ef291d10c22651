"""Box NMS on an object table: de-duplication by the yaw-oriented boxes of ``describe_instances`` where the masks are
gone -- a ``load_objects`` file, a table merged from tiles.  The reference has no counterpart; the rules are those of
``softgroup_amd.ops.boxes``: descending ``conf`` (as float32), the LOWER index first among equal scores, a kept box
suppresses the later boxes of its ``label_id`` (any label when class-agnostic) whose IoU exceeds ``thr``, strictly.

backends (both produce the same flags)
  'numpy'   ``box_nms_numpy``
  'device'  ``sg_box_nms`` on the uploaded rows, one read-back of the keep flags and the flag word; at most 16 384 rows
  'auto'    numpy without a GPU; with one, what ``ops.boxes._AUTO['nms']`` says; beyond the device's range numpy
"""
import numpy as np

from ..ops import boxes as BX
from .objects import ObjectTable

__all__ = ['nms_boxes', 'take_rows', 'nms_objects']


def _keep_device(rows, scores, labels, thr, mode, class_agnostic):
    import torch
    dev = torch.device('cuda', torch.cuda.current_device())
    keep, n_keep = BX.box_nms(torch.from_numpy(rows).to(dev), torch.from_numpy(scores).to(dev),
                              torch.from_numpy(labels).to(dev), thr, mode, class_agnostic)
    back = torch.cat([keep.to(torch.int32), n_keep]).cpu().numpy()
    BX._flags_raise(back[-1], 'nms_boxes')
    return back[:-2].astype(np.uint8)


def nms_boxes(table, thr=0.25, mode='3d', class_agnostic=False, backend='auto'):
    """keep flags, bool [n], of the rows of an ``ObjectTable`` (``obb``, ``conf``, ``label_id``) that survive greedy
    box NMS.  Rows with ``npoint == 0`` (their boxes are NaN) are dropped first and are never passed on."""
    BX._mode(mode)
    chosen = BX.auto_backend(backend, 'nms')
    for key in ('obb', 'conf', 'label_id'):
        if key not in table:
            raise ValueError(f'nms_boxes: a table with {key!r}')
    obb = np.asarray(table['obb'], np.float64).reshape(-1, 7)
    n = obb.shape[0]
    some = np.asarray(table['npoint']).reshape(-1) != 0 if 'npoint' in table else np.ones(n, bool)
    scores = np.asarray(table['conf'], np.float64).reshape(-1).astype(np.float32)
    labels = np.asarray(table['label_id']).reshape(-1).astype(np.int64).astype(np.int32)
    if scores.shape[0] != n or labels.shape[0] != n or some.shape[0] != n:
        raise ValueError('nms_boxes: columns of different lengths')
    if not np.isfinite(scores[some]).all():
        raise ValueError('nms_boxes: scores must be finite')
    idx = np.flatnonzero(some)
    rows = BX.boxes8(obb[idx])
    BX._check(rows, 'nms_boxes')
    args = (rows, np.ascontiguousarray(scores[idx]), np.ascontiguousarray(labels[idx]), float(thr), mode,
            bool(class_agnostic))
    if chosen == 'device' and idx.size > BX.MAX_NMS_BOXES:
        if backend != 'auto':
            from .. import _lib as L
            raise L.SoftGroupHipError(f'nms_boxes: {idx.size} boxes: outside the supported range (at most '
                                      f'{BX.MAX_NMS_BOXES})')
        chosen = 'numpy'
    kept = _keep_device(*args) if chosen == 'device' else BX.box_nms_numpy(*args)[0]
    keep = np.zeros(n, dtype=bool)
    keep[idx] = kept != 0
    return keep


def take_rows(table, keep):
    """the table with the rows of ``keep`` (bool [n] or indices) in every column"""
    keep = np.asarray(keep)
    return ObjectTable((key, np.asarray(col)[keep]) for key, col in table.items())


def nms_objects(pred_instances, table, thr=0.25, mode='3d', class_agnostic=False, backend='auto'):
    """-> (the instances that survive ``nms_boxes`` on their table -- the same dict objects in the same order --, the
    table of those rows)"""
    insts = list(pred_instances)
    keep = nms_boxes(table, thr, mode, class_agnostic, backend)
    if len(insts) != keep.shape[0]:
        raise ValueError(f'nms_objects: {len(insts)} instances for a table of {keep.shape[0]} rows')
    return [inst for inst, k in zip(insts, keep) if k], take_rows(table, keep)
