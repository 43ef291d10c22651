"""The object table of an instance list: for every mask of what ``SoftGroup.get_instances`` / ``load_pred_instances``
/ ``stitch_results`` / ``ensemble_results`` return, how many points it has, where it is, how big, which way it faces,
what colour it is and how pure its semantic vote is.  The reference has no counterpart.  Nothing in ``forward_test``
or ``ScanForward`` calls this stage.

rules (include/softgroup_hip.h, ``softgroup_amd.ops.objects``; the numpy backend is the definition)
  * ``npoint``, ``aabb`` = (xmin, ymin, zmin, xmax, ymax, zmax), ``centroid``, ``cov6`` = the centred second moments
    (xx, xy, xz, yy, yz, zz) divided by ``npoint``, ``mean_color``: float64, sums in the fixed order of the ops module;
  * ``obb`` = (cx, cy, cz, du, dv, dz, theta): the enclosing rectangle of smallest area in the xy plane over the
    ``yaw_steps`` directions ``theta_a = a * (pi / 2) / yaw_steps`` (the lowest index among equal areas), with
    ``refine = r > 0`` a second sweep over ``theta_best + j * step / (r + 1)``, j = -r .. r; ``du`` lies along
    ``(cos theta, sin theta)``, ``dv`` along ``(-sin theta, cos theta)``; ``theta`` is not wrapped; ``angle_index`` is
    the coarse winner;
  * ``sem_label`` / ``sem_count``: the class in ``0 .. n_classes-1`` that most mask points carry in ``semantic`` (the
    lowest among equal counts) and that count; ``-1 / 0`` for a mask without a counted label;
  * an empty mask: ``npoint`` 0, every float NaN, ``angle_index`` -1, ``sem_label`` -1;
  * a point of at least one mask whose coordinate (or colour) is not finite raises ``ValueError``; a non-finite value at
    a point that is in no mask is never an error.

backends (both produce the same bytes)
  'numpy'   packed rows (``util/masks.py``) and the twins of ``ops/objects.py``
  'device'  RLE text -> bit rows on the device -> ``sg_instance_moments``, ``sg_instance_extents`` (twice with
            ``refine``: the per-mask tables are gathered on the device by the coarse winner), ``sg_instance_class_hist``
            -> ONE read-back of everything, the flags included -> box composition on the host.  Range: 16 384 masks,
            fewer than 2**31 points, 256 classes.
  'auto'    numpy without a GPU; with one, what ``ops.objects._AUTO`` says; beyond the device's range and for RLE
            strings whose runs are not ascending ``'auto'`` takes numpy, ``'device'`` raises.
"""
import json

import numpy as np

from ..ops import objects as OB
from ..ops._args import _host, _words
from . import masks as M
from .lazy import LazyResults

__all__ = ['ObjectTable', 'describe_instances', 'describe_result', 'box_corners', 'save_objects', 'load_objects']

_FORMAT = 'softgroup_amd.objects/1'


class ObjectTable(dict):
    """a dict of numpy arrays with one row per instance"""


class _OutOfRange(Exception):
    pass


def _carry(table, insts):
    if insts and all('scan_id' in i for i in insts):
        table['scan_id'] = np.array([str(i['scan_id']) for i in insts])
    if insts and all('label_id' in i for i in insts):
        table['label_id'] = np.array([int(i['label_id']) for i in insts], dtype=np.int64)
    if insts and all('conf' in i for i in insts):
        table['conf'] = np.array([float(i['conf']) for i in insts], dtype=np.float64)
    return table


def _finish(insts, parts, yaw_steps, refine):
    """host arrays of both backends -> the table: the chosen angle's (theta, cos, sin) and the box composition"""
    if int(parts['flags']) & OB.FLAG_NOT_FINITE:
        raise ValueError('describe_instances: a coordinate or colour of a mask point is not finite')
    coarse = parts['angle_index'].astype(np.int64)
    some = coarse >= 0
    n = coarse.size
    theta, cs = np.full(n, np.nan), np.full((n, 2), np.nan)
    if refine:
        fine_theta, fine_tab = OB.refine_tables(yaw_steps, refine)
        fine = parts['fine_index'].astype(np.int64)
        theta[some], cs[some] = fine_theta[coarse[some], fine[some]], fine_tab[coarse[some], fine[some]]
    else:
        all_theta, tab = OB.yaw_table(yaw_steps)
        theta[some], cs[some] = all_theta[coarse[some]], tab[coarse[some]]
    table = ObjectTable(npoint=parts['npoint'].astype(np.int32), aabb=parts['aabb'], centroid=parts['centroid'],
                        cov6=parts['cov6'],
                        obb=OB.compose_boxes(parts['ext'], cs, theta, parts['aabb'][:, 2], parts['aabb'][:, 5]),
                        angle_index=coarse.astype(np.int32))
    for key in ('mean_color', 'sem_label', 'sem_count'):
        if key in parts:
            table[key] = parts[key] if key == 'mean_color' else parts[key].astype(np.int32)
    return _carry(table, insts)


def _describe_numpy(insts, n_points, coords, colors, semantic, n_classes, yaw_steps, refine):
    rows = M.packed_rows(insts, n_points).view(np.uint32).reshape(len(insts), _words(n_points))
    xyz = np.ascontiguousarray(_host(coords), dtype=np.float32)
    rgb = None if colors is None else np.ascontiguousarray(_host(colors), dtype=np.float32)
    mo = OB.instance_moments_numpy(rows, n_points, xyz, rgb)
    ex = OB.instance_extents_numpy(rows, n_points, xyz, OB.yaw_table(yaw_steps)[1])
    parts = {k: mo[k] for k in ('npoint', 'aabb', 'centroid', 'cov6')}
    parts.update(angle_index=ex['best_index'], ext=ex['best_ext'], flags=mo['flags'] | ex['flags'])
    if refine:
        tabs = OB.refine_tables(yaw_steps, refine)[1][np.maximum(ex['best_index'], 0)]
        ex2 = OB.instance_extents_numpy(rows, n_points, xyz, tabs, 2 * refine + 1)
        parts.update(fine_index=ex2['best_index'], ext=ex2['best_ext'], flags=parts['flags'] | ex2['flags'])
    if rgb is not None:
        parts['mean_color'] = mo['mean_color']
    if semantic is not None:
        hist = OB.instance_class_hist_numpy(rows, n_points, _host(semantic).reshape(-1), n_classes)
        parts.update(sem_label=hist['sem_label'], sem_count=hist['sem_count'])
    return _finish(insts, parts, yaw_steps, refine)


def _on_device(a, dev, dtype=None):
    import torch
    if not torch.is_tensor(a):
        a = np.ascontiguousarray(a)
        a = torch.from_numpy(a if a.flags.writeable else a.copy())
    a = a.detach().to(dev)
    return a if dtype is None else a.to(dtype)


def _describe_device(insts, n_points, coords, colors, semantic, n_classes, yaw_steps, refine):
    import torch
    n = len(insts)
    if n > OB.MAX_INSTANCES or n_points >= OB.MAX_DEVICE_POINTS or (semantic is not None
                                                                     and n_classes > OB.MAX_CLASSES):
        raise _OutOfRange(f'{n} masks over {n_points} points' + (f', {n_classes} classes' if semantic is not None
                                                                  else ''))
    dev = torch.device('cuda', torch.cuda.current_device())
    with torch.cuda.device(dev):
        bits, check = M.rows_device(insts, n_points, dev)
        xyz = _on_device(coords, dev, torch.float32)
        rgb = None if colors is None else _on_device(colors, dev, torch.float32)
        mo = OB.instance_moments(bits, n_points, xyz, rgb)
        ex = OB.instance_extents(bits, n_points, xyz, OB.yaw_table(yaw_steps)[1])
        names = ['npoint', 'aabb', 'centroid', 'cov6', 'angle_index', 'ext']
        cols = [mo['npoint'], mo['aabb'], mo['centroid'], mo['cov6'], ex['best_index'], ex['best_ext']]
        flags = mo['flags'] | ex['flags']
        if refine:
            tabs = _on_device(OB.refine_tables(yaw_steps, refine)[1], dev)[ex['best_index'].clamp(min=0).long()]
            ex2 = OB.instance_extents(bits, n_points, xyz, tabs.contiguous(), 2 * refine + 1)
            cols[5] = ex2['best_ext']
            names.append('fine_index'), cols.append(ex2['best_index'])
            flags = flags | ex2['flags']
        if rgb is not None:
            names.append('mean_color'), cols.append(mo['mean_color'])
        if semantic is not None:
            lab = _on_device(semantic, dev).reshape(-1)
            if lab.is_floating_point():
                raise ValueError('semantic: integer labels')
            hist = OB.instance_class_hist(bits, n_points, lab, n_classes)
            names += ['sem_label', 'sem_count']
            cols += [hist['sem_label'], hist['sem_count']]
        names.append('flags'), cols.append(flags)
        if check is not None:
            names.append('check'), cols.append(check)
        # the one read-back: int32 values are exact in float64, the float64 columns travel as they are
        back = torch.cat([c.reshape(-1).to(torch.float64) for c in cols]).cpu().numpy()
    parts, at = {}, 0
    for name, col in zip(names, cols):
        parts[name] = back[at:at + col.numel()].reshape(tuple(col.shape))
        at += col.numel()
    if 'check' in parts:
        M.raise_bad_rle(bool(parts['check'][0]), bool(parts['check'][1]))
    for name in ('npoint', 'angle_index', 'fine_index', 'sem_label', 'sem_count', 'flags'):
        if name in parts:
            parts[name] = parts[name].astype(np.int64)
    parts['flags'] = int(parts['flags'][0])
    return _finish(insts, parts, yaw_steps, refine)


def _n_rows(a):
    return int(a.shape[0])


def _array(a):
    import torch
    return a if a is None or torch.is_tensor(a) else np.asarray(a)


def describe_instances(pred_instances, coords, colors=None, semantic=None, n_classes=None, yaw_steps=90, refine=0,
                       backend='auto'):
    """-> an ``ObjectTable`` (a dict of numpy arrays, one row per instance): ``npoint``, ``aabb``, ``centroid``,
    ``cov6``, ``obb``, ``angle_index``; with ``colors`` also ``mean_color``, with ``semantic`` (and ``n_classes``)
    ``sem_label`` and ``sem_count``; ``scan_id``, ``label_id`` and ``conf`` where every instance has them.
    ``pred_instances``: dicts whose ``pred_mask`` is an RLE dict or a dense array over the points of ``coords``
    (float [N, 3], numpy or torch, host or device).  See the module text for the rules."""
    yaw_steps, refine = OB._yaw_steps(yaw_steps), OB._refine(refine)
    if semantic is not None:
        n_classes = OB._n_classes(n_classes)
    chosen = OB.auto_backend(backend, 'describe')
    insts = list(pred_instances)
    coords, colors, semantic = _array(coords), _array(colors), _array(semantic)
    if len(coords.shape) != 2 or coords.shape[1] != 3:
        raise ValueError('coords: an array [N, 3]')
    n_points = M.mask_length(insts) if insts else _n_rows(coords)
    if _n_rows(coords) != n_points:
        raise ValueError(f'coords: {_n_rows(coords)} points for masks of {n_points}')
    if colors is not None and (len(colors.shape) != 2 or colors.shape[1] != 3 or _n_rows(colors) != n_points):
        raise ValueError(f'colors: an array [{n_points}, 3]')
    if semantic is not None and int(np.prod(tuple(semantic.shape))) != n_points:
        raise ValueError(f'semantic: {n_points} labels, one per point')
    args = (insts, n_points, coords, colors, semantic, n_classes, yaw_steps, refine)
    if not insts:
        return _describe_numpy(*args)

    def device(*a):
        try:
            return _describe_device(*a)
        except _OutOfRange as e:
            if backend != 'auto':
                from .. import _lib as L
                raise L.SoftGroupHipError(f'describe_instances: {e}: outside the supported range (at most '
                                          f'{OB.MAX_INSTANCES} masks, fewer than 2**31 points, at most '
                                          f'{OB.MAX_CLASSES} classes)')
            return _describe_numpy(*a)

    return M.with_fallback(backend, chosen, device, _describe_numpy, *args)


def describe_result(result, n_classes=None, yaw_steps=90, refine=0, backend='auto'):
    """``describe_instances`` on a result dict of ``forward_test`` (a lazy result is resolved first): the masks of
    ``pred_instances`` over ``coords_float``, with ``color_feats`` and -- when ``n_classes`` is given --
    ``semantic_preds`` where the result has them"""
    if isinstance(result, LazyResults):
        result.resolve()
    if 'pred_instances' not in result or 'coords_float' not in result:
        raise ValueError('describe_result: a result with pred_instances and coords_float')
    semantic = result.get('semantic_preds') if n_classes is not None else None
    return describe_instances(result['pred_instances'], result['coords_float'], result.get('color_feats'), semantic,
                              n_classes if semantic is not None else None, yaw_steps, refine, backend)


def box_corners(obb):
    """obb [n, 7] (or a table) -> float64 [n, 8, 3]: corner ``4 k + 2 j + i`` lies at ``(-1)^(1-i) du / 2`` along
    (cos theta, sin theta), ``(-1)^(1-j) dv / 2`` along (-sin theta, cos theta) and ``(-1)^(1-k) dz / 2`` along z"""
    obb = np.asarray(obb['obb'] if isinstance(obb, dict) else obb, dtype=np.float64).reshape(-1, 7)
    c, s = np.cos(obb[:, 6]), np.sin(obb[:, 6])
    out = np.empty((obb.shape[0], 8, 3), np.float64)
    for k in range(2):
        for j in range(2):
            for i in range(2):
                hu, hv = (i - 0.5) * obb[:, 3], (j - 0.5) * obb[:, 4]
                out[:, 4 * k + 2 * j + i, 0] = obb[:, 0] + hu * c - hv * s
                out[:, 4 * k + 2 * j + i, 1] = obb[:, 1] + hu * s + hv * c
                out[:, 4 * k + 2 * j + i, 2] = obb[:, 2] + (k - 0.5) * obb[:, 5]
    return out


# ---- files -----------------------------------------------------------------------------------------------------------
def _plain(v):
    if isinstance(v, float):
        return None if v != v else v
    return v


def save_objects(path, table):
    """the table as JSON: per column its dtype, shape and flat values; NaN is written as ``null``, floats in Python's
    shortest round-trip form, so that ``load_objects`` returns the same bytes"""
    cols = {}
    for key, a in table.items():
        a = np.asarray(a)
        cols[key] = {'dtype': a.dtype.str, 'shape': list(a.shape),
                     'values': [_plain(v) for v in a.reshape(-1).tolist()]}
    with open(path, 'w') as f:
        json.dump({'format': _FORMAT, 'columns': cols}, f)
        f.write('\n')


def load_objects(path):
    """the table ``save_objects`` wrote"""
    with open(path) as f:
        doc = json.load(f)
    if doc.get('format') != _FORMAT:
        raise ValueError(f'{path}: not an object table ({_FORMAT})')
    table = ObjectTable()
    for key, col in doc['columns'].items():
        dtype = np.dtype(col['dtype'])
        values = col['values']
        if dtype.kind == 'f':
            values = [np.nan if v is None else v for v in values]
        table[key] = np.array(values, dtype=dtype).reshape(col['shape'])
    return table
