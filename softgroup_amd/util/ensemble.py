"""Several results over the SAME points combined into one: the rotated and mirrored passes of test-time augmentation
(``softgroup_amd.data.tta_scan``), the folds or seeds of several checkpoints, a tiled-and-stitched result next to a
thinned-and-propagated one.  The reference has no counterpart.  ``stitch_results`` cannot stand in: its masks live on
different point lists, and it unions members, which is right for two halves of one object and wrong for K opinions
about one object.

rules (include/softgroup_hip.h, ``softgroup_amd.ops.ensemble``; the numpy backend is the definition)
  * ``results[p]`` is the result dict of pass p over the same N points in the same order (lazy results are resolved
    first); 1 <= K <= 32 passes; pass p has an integer weight ``w_p >= 1`` (default 1), ``W = sum w_p <= 32767``; the
    inputs are not modified; a per-point array or a mask of another length than pass 0's raises ``ValueError``, and
    so does a key that one pass has and another lacks;
  * ``semantic_preds`` is the LABEL VOTE: a label is counted when it is ``>= 0`` and ``!= ignore_label``; the class
    with the greatest summed weight wins, the lowest class among equal sums; a point with no counted label keeps
    pass 0's value; the array keeps pass 0's dtype and location;
  * instances are numbered g = 0 .. G-1 by (pass, list order); two instances of DIFFERENT passes with equal
    ``label_id`` are LINKED when ``inter >= min_shared``, ``den > 0`` and ``float64(inter) / float64(den) > thr``,
    strictly, ``den = ca + cb - inter`` ('iou') or ``min(ca, cb)`` ('min'), populations over all N points -- the rule
    of ``stitch_results``; an OBJECT is a connected component of the links; its SUPPORT ``s`` is the sum of ``w_p``
    over the distinct passes that have a member in it;
  * an object is kept when ``s >= min_votes`` (default ``W // 2 + 1``, in 1 .. W);
  * its mask is the MASK VOTE: at a point, ``v`` = the sum of ``w_p`` over the passes with at least one member that
    holds the point (a pass counts once); the point is in when ``v >= need``, ``need = s // 2 + 1`` for
    ``mask='majority'`` (``2 v > s``), 1 for ``'union'``, ``s`` for ``'all'``; an object whose voted mask has fewer
    than ``min_npoint`` points is dropped;
  * ``label_id`` is the common label, ``scan_id`` and every other key come from the first member; ``conf`` is, in
    float64 on the host for both backends, the sum over the passes p with a member, in ascending p, of
    ``w_p * (the greatest conf of the object's members in p)``, divided by ``float64(W)``: an object that only half
    the passes see scores lower; ``pred_mask`` is a canonical RLE dict of ``length = N`` (a bool array when the first
    member's mask was a dense array); the output order is ascending smallest member;
  * ``panoptic_preds`` is DROPPED: its ids are per pass (the rule of ``stitch_results``); ``offset_preds``,
    ``coords_float``, the label arrays and every other key are copied from ``results[0]`` -- by convention the
    untransformed pass; the offsets of a rotated pass are rotated vectors and are not averaged.

backends (both produce the same strings, labels and scores)
  'numpy'   packed rows of all passes stacked, popcounts, a union-find, a dense count per object
  'device'  RLE text -> one stacked bit matrix (the route of ``util/masks.py``) -> ``sg_mask_group_links`` ->
            ``sg_stitch_components`` -> ONE small read-back (components and the RLE check flags) -> objects, support
            and need on the host, O(G) -> ``sg_mask_vote`` -> ``sg_mask_runs_count`` / ``_fill`` ->
            ``sg_rle_format_device`` (the populations ride with its text offsets); labels through ``sg_label_vote``,
            which never synchronises.  Range: G <= 16384 instances, N < 2**31.
  'auto'    numpy without a GPU; with one, what ``ops.ensemble._AUTO`` says per operation; beyond the device's range
            and for RLE strings whose runs are not ascending ``'auto'`` takes numpy, ``'device'`` raises.
"""
import numpy as np

from ..ops import ensemble as EN
from ..ops import resample as RS
from ..ops import stitch as ST
from ..ops._args import _host
from . import masks as M
from .lazy import LazyResults

__all__ = ['ensemble_results']

_DROPPED = ('panoptic_preds', )
# the keys whose first dimension is the point
_PER_POINT = ('semantic_preds', 'offset_preds', 'panoptic_preds', 'coords_float', 'semantic_labels', 'instance_labels',
              'offset_labels', 'color_feats', 'semantic_scores')
_NEED = ('majority', 'union', 'all')


class _OutOfRange(Exception):
    pass


def _vote_labels(values, weights, ignore_label, backend):
    import torch
    first = values[0]
    chosen = EN.auto_backend(backend, 'labels')
    n = int(first.shape[0])
    if chosen == 'device' and n >= EN.MAX_DEVICE_POINTS:
        if backend != 'auto':
            from .. import _lib as L
            raise L.SoftGroupHipError(f'ensemble_results: {n} points: outside the supported range (N < 2**31)')
        chosen = 'numpy'
    on_device = torch.is_tensor(first) and first.is_cuda
    if chosen == 'device':
        dev = first.device if on_device else torch.device('cuda', torch.cuda.current_device())
        rows = torch.stack([(v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))).to(dev).long()
                            .reshape(-1) for v in values])
        out = EN.label_vote(rows, weights, ignore_label)
        if on_device:
            return out.to(first.dtype)
        return out.cpu().to(first.dtype) if torch.is_tensor(first) else out.cpu().numpy().astype(first.dtype)
    out = EN.label_vote_numpy(np.stack([_host(v).reshape(-1).astype(np.int64) for v in values]), weights,
                              ignore_label)
    if torch.is_tensor(first):
        return torch.from_numpy(out).to(first.dtype).to(first.device)
    return out.astype(np.asarray(first).dtype)


def _need(support, mask):
    return {'majority': support // 2 + 1, 'union': np.ones_like(support), 'all': support}[mask]


def _kept_objects(comp, group, weights, min_votes, mask):
    """-> (member lists of the objects with enough support, in output order; need int64 per object)"""
    objects, support = EN.objects_of_components(comp, group, weights)
    keep = np.flatnonzero(support >= min_votes)
    return [objects[o] for o in keep.tolist()], _need(support[keep], mask)


def _conf(members, insts, group, weights):
    total = np.float64(int(weights.sum()))
    acc = np.float64(0.0)
    for p in sorted({int(group[g]) for g in members}):
        acc = acc + np.float64(int(weights[p])) * max(np.float64(insts[g]['conf']) for g in members if group[g] == p)
    return float(acc / total)


def _merged(objects, insts, group, weights, masks):
    out = []
    for m, mask in zip(objects, masks):
        first = insts[m[0]]
        new = dict(first, pred_mask=mask)
        if all('conf' in insts[g] for g in m):
            new['conf'] = _conf(m, insts, group, weights)
        out.append(new)
    return out


def _host_masks(objects, insts, bits_host, n_points):
    """output masks from voted rows on the host: RLE for an object whose first member was RLE, a bool array otherwise"""
    if not objects:
        return []
    rows = np.ascontiguousarray(bits_host).view(np.uint8).reshape(len(objects), -1)
    rle = [None] * len(objects)
    if any(isinstance(insts[m[0]]['pred_mask'], dict) for m in objects):
        rle = M.rle_dicts_from_bits_numpy(rows, n_points)
    return [rle[o] if isinstance(insts[m[0]]['pred_mask'], dict) else
            np.unpackbits(rows[o], bitorder='little')[:n_points].astype(bool) for o, m in enumerate(objects)]


def _ensemble_numpy(per_pass, insts, labels, group, weights, n_points, thr, measure, min_shared, min_votes, mask,
                    min_npoint):
    rows = np.concatenate([M.packed_rows(pi, n_points) for pi in per_pass])
    adj = EN.mask_group_links_numpy(rows, n_points, labels, group, thr, measure, min_shared)
    comp = ST.stitch_components_numpy(adj, len(insts))
    objects, need = _kept_objects(comp, group, weights, min_votes, mask)
    obj_of = np.full(len(insts), -1, np.int64)
    for o, m in enumerate(objects):
        obj_of[m] = o
    out_bits, npoint = EN.mask_vote_numpy(rows, n_points, obj_of, group, weights, need)
    keep = np.flatnonzero(npoint >= min_npoint).tolist()
    objects = [objects[o] for o in keep]
    return _merged(objects, insts, group, weights, _host_masks(objects, insts, out_bits[keep], n_points))


def _ensemble_device(per_pass, insts, labels, group, weights, n_points, thr, measure, min_shared, min_votes, mask,
                     min_npoint):
    import torch
    dev = torch.device('cuda', torch.cuda.current_device())
    n_total = len(insts)
    if n_total > EN.MAX_INSTANCES or n_points >= EN.MAX_DEVICE_POINTS:
        raise _OutOfRange(f'{n_total} instances over {n_points} points')
    with torch.cuda.device(dev):
        bits, checks = [], []
        for pi in per_pass:
            if pi:
                b, check = M.rows_device(pi, n_points, dev)
                bits.append(b)
                if check is not None:
                    checks.append(check)
        bits = torch.cat(bits) if len(bits) > 1 else bits[0]
        adj = EN.mask_group_links(bits, n_points, labels, group, thr, measure, min_shared)
        comp = ST.stitch_components(adj, n_total)
        check = torch.stack(checks).any(0).int() if checks else torch.zeros(2, dtype=torch.int32, device=dev)
        back = torch.cat([comp, check]).cpu().numpy()               # the one small read-back
        M.raise_bad_rle(back[n_total], back[n_total + 1])
        objects, need = _kept_objects(back[:n_total], group, weights, min_votes, mask)
        if not objects:
            return []
        all_rle = all(isinstance(insts[m[0]]['pred_mask'], dict) for m in objects)
        if all_rle and not RS.mask_runs_supported(len(objects), n_points):
            raise _OutOfRange(f'{len(objects)} objects over {n_points} points (more runs than int32 numbers)')
        out_bits, npoint = EN.mask_vote(bits, n_points, *EN.member_lists(objects, group, weights), need)
        if not all_rle:
            npoint, out_bits = npoint.cpu().numpy(), out_bits.cpu().numpy()
            keep = np.flatnonzero(npoint >= min_npoint).tolist()
            objects = [objects[o] for o in keep]
            return _merged(objects, insts, group, weights, _host_masks(objects, insts, out_bits[keep], n_points))
        starts, ends, bounds = RS.mask_runs_from_bits(out_bits, n_points)
        masks, npoint = M.rle_dicts_from_runs_device(starts, ends, bounds, len(objects), n_points, dev, extra=npoint)
    keep = [o for o in range(len(objects)) if npoint[o] >= min_npoint]
    return _merged([objects[o] for o in keep], insts, group, weights, [masks[o] for o in keep])


def ensemble_results(results, weights=None, thr=0.5, measure='iou', min_shared=1, min_votes=None, mask='majority',
                     min_npoint=0, ignore_label=-100, backend='auto'):
    """-> a NEW result dict: the K results of ``results`` (dicts of ``forward_test`` / ``ScanForward`` over the same
    points in the same order) combined into one (see the module text).  ``weights``: one integer >= 1 per pass;
    ``min_votes``: the support an object needs, default ``W // 2 + 1``; ``mask``: 'majority', 'union' or 'all'.
    ``panoptic_preds`` is dropped: its ids are per pass."""
    from ..ops.nms import _measure
    _measure(measure)
    if mask not in _NEED:
        raise ValueError(f"mask {mask!r}: one of 'majority', 'union', 'all'")
    if int(min_npoint) != min_npoint or int(min_npoint) < 0:
        raise ValueError(f'min_npoint {min_npoint!r}: an integer >= 0')
    chosen = EN.auto_backend(backend, 'instances')
    if isinstance(results, LazyResults):
        results.resolve()
    results = list(results)
    for r in results:
        if isinstance(r, LazyResults):
            r.resolve()
    weights = EN.pass_weights(weights, len(results))
    total = int(weights.sum())
    if min_votes is None:
        min_votes = total // 2 + 1
    if int(min_votes) != min_votes or not 1 <= int(min_votes) <= total:
        raise ValueError(f'min_votes {min_votes!r}: an integer between 1 and the sum of the weights, {total}')
    first = results[0]
    keys = set(dict.keys(first))
    for p, r in enumerate(results):
        odd = keys ^ set(dict.keys(r))
        if odd:
            raise ValueError(f'{sorted(odd)[0]}: in the result of one of the passes 0 and {p} but not of the other')
    # the number of points: every per-point array and every mask of every pass agrees with pass 0's
    n_points = None
    for p, r in enumerate(results):
        for key in _PER_POINT:
            if key in keys and hasattr(r[key], 'shape'):
                k = int(r[key].shape[0])
                n_points = k if n_points is None else n_points
                if k != n_points:
                    raise ValueError(f'{key}: {k} entries in the result of pass {p}, pass 0 has {n_points} points')
    per_pass = [list(r['pred_instances']) for r in results] if 'pred_instances' in keys else None
    for p, pi in enumerate(per_pass or []):
        if pi:
            k = M.mask_length(pi)
            n_points = k if n_points is None else n_points
            if k != n_points:
                raise ValueError(f'pred_instances of pass {p}: masks of {k} points, pass 0 has {n_points}')
    out = {}
    for key, value in dict.items(first):
        if key == 'semantic_preds':
            out[key] = _vote_labels([r[key] for r in results], weights, int(ignore_label), backend)
        elif key in _DROPPED or key == 'pred_instances':
            pass
        else:
            out[key] = value
    if per_pass is None:
        return out
    insts = [inst for pi in per_pass for inst in pi]
    group = np.repeat(np.arange(len(per_pass)), [len(pi) for pi in per_pass]).astype(np.int32)
    labels = np.array([int(inst['label_id']) for inst in insts], dtype=np.int64).astype(np.int32)
    args = (per_pass, insts, labels, group, weights, n_points, float(thr), measure, int(min_shared), int(min_votes), mask,
            int(min_npoint))

    def device(*a):
        try:
            return _ensemble_device(*a)
        except _OutOfRange as e:
            if backend != 'auto':
                from .. import _lib as L
                raise L.SoftGroupHipError(f'ensemble_results: {e}: outside the supported range (at most '
                                          f'{EN.MAX_INSTANCES} instances, fewer than 2**31 points)')
            return _ensemble_numpy(*a)

    out['pred_instances'] = M.with_fallback(backend, chosen, device, _ensemble_numpy, *args) if insts else []
    return out
