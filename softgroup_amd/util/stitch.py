"""The results of the tiles of one large cloud (``softgroup_amd.data.tile_cloud``) joined into one result over the
full cloud: what follows the scans of ``xyz[ids] for ids in tiles.point_ids`` so that ``save_results``, the
evaluators and ``nms_instances`` get one entry per original point and one instance per object.  The reference has no
counterpart (it evaluates every block as a scene of its own).

rules (include/softgroup_hip.h, ``softgroup_amd.ops.stitch``; the numpy backend is the definition)
  * ``results[t]`` is the result dict of tile t over its ``len(tiles.point_ids[t])`` points (lazy results are
    resolved first); a per-point array or a mask of another length raises ``ValueError``; the inputs are not modified;
  * ``semantic_preds`` and ``offset_preds`` take their value at point p from p's core tile:
    ``results[core_tile[p]][key][core_pos[p]]``;
  * ``panoptic_preds`` is DROPPED: its ids are numbered per tile and nothing here renumbers them;
  * ``coords_float`` becomes ``coords`` when given and is dropped otherwise; ``semantic_labels``,
    ``instance_labels``, ``offset_labels``, ``color_feats``, ``gt_instances`` are taken from ``gt`` when it has them
    and dropped otherwise (the rules of ``propagate_result``); every other key is copied from ``results[0]``;
  * tile instances are numbered g = 0 .. G-1 by tile, then by list order; M(g) = the global ids
    ``point_ids[t][mask positions]``;
  * two instances g, h of different, neighbouring tiles a, b with equal ``label_id`` are LINKED when, with S = the
    points in both tiles' lists, ``ca = |M(g) & S|``, ``cb = |M(h) & S|``, ``inter = |M(g) & M(h)|``,
    ``den = ca + cb - inter`` ('iou') or ``min(ca, cb)`` ('min'): ``inter >= min_shared``, ``den > 0`` and
    ``float64(inter) / float64(den) > thr``, strictly (one IEEE division, the rule of ``sg_mask_nms``);
  * an OBJECT is a connected component of the link graph.  Links are transitive: two instances of ONE tile can end
    up in one object through a neighbour's instance that overlaps both (``nms_instances`` may follow to prune what
    the tiles' own scans left as duplicates).  Its mask is the union of its members' M, its ``label_id`` the common
    one, its ``conf`` the maximum of its members', its ``scan_id`` (and every other key) that of its first member;
    the output order is ascending smallest member g;
  * ``drop_margin_only``: a component of ONE instance whose M holds no core point of its own tile is dropped (an
    empty mask holds none) -- the neighbour that owns those points sees the object whole; unlinked, the instance is
    a truncated duplicate or nothing;
  * ``pred_mask`` is a canonical RLE dict of ``length = N``, byte for byte ``rle_encode`` of the dense union.

backends (both produce the same strings)
  'numpy'   packed rows per tile, popcounts, a union-find and one sort of the (object, id) pairs on the host
  'device'  RLE text -> bit rows per tile (the route of ``util/masks.py``) -> ``sg_tile_shared`` ->
            ``sg_mask_bits_gather`` onto the shared strip -> ``sg_mask_cross_links`` -> ``sg_stitch_components`` ->
            ``sg_mask_bits_ids_count`` / ``_fill`` -> ``sg_stitch_union_count`` / ``_fill`` ->
            ``sg_rle_format_device``.  No row over the full cloud exists: memory is the tiles' own bit rows plus
            24 bytes per mask point.  Range: G <= 16384 tile instances, sum |M(g)| < 2**31, N < 2**31.  Read-backs:
            the shared counts (all pairs at once), the component numbers with the populations, the run total, the text.
  'auto'    numpy without a GPU; with one, what ``ops.stitch._AUTO['stitch']`` says; beyond the device's range and
            for RLE strings whose runs are not ascending ``'auto'`` takes numpy, ``'device'`` raises.
"""
import numpy as np

from ..ops import resample as RS
from ..ops import stitch as ST
from ..ops._args import _host
from . import masks as M
from .lazy import LazyResults

__all__ = ['stitch_results']

_FROM_CORE = ('semantic_preds', 'offset_preds')
_DROPPED = ('panoptic_preds', )


class _OutOfRange(Exception):
    pass


def _from_core(results, key, tiles, n_tile):
    """value at point p = results[core_tile[p]][key][core_pos[p]]: one concatenation, one gather"""
    import torch
    vals = []
    for t, r in enumerate(results):
        if key not in r:
            raise ValueError(f'{key}: in the result of tile 0 but not of tile {t}')
        if int(r[key].shape[0]) != n_tile[t]:
            raise ValueError(f'{key}: {r[key].shape[0]} entries in the result of tile {t}, which has {n_tile[t]} points')
        vals.append(r[key])
    if any(torch.is_tensor(v) for v in vals):
        dev = next(v.device for v in vals if torch.is_tensor(v))
        big = torch.cat([torch.as_tensor(v).to(dev) for v in vals])
        off = torch.as_tensor(np.asarray(tiles.offsets[:-1], np.int64)).to(dev)
        core_tile = torch.as_tensor(tiles.core_tile).to(dev).long()
        return big[off[core_tile] + torch.as_tensor(tiles.core_pos).to(dev).long()]
    big = np.concatenate([np.asarray(v) for v in vals])
    off = np.asarray(tiles.offsets[:-1], np.int64)
    return big[off[_host(tiles.core_tile).astype(np.int64)] + _host(tiles.core_pos).astype(np.int64)]


def _objects(comp, core_cnt, insts, drop):
    """-> (members of every kept object in output order, object number of every tile instance or -1)"""
    members = {}
    for g, root in enumerate(comp):
        members.setdefault(int(root), []).append(g)
    objects, key = [], np.full(len(insts), -1, np.int32)
    for root in sorted(members):
        m = members[root]
        if drop and len(m) == 1 and int(core_cnt[m[0]]) == 0:
            continue
        key[m] = len(objects)
        objects.append(m)
    return objects, key


def _merged(objects, insts, masks):
    out = []
    for m, mask in zip(objects, masks):
        first = insts[m[0]]
        out.append(dict(first, label_id=first['label_id'], conf=max(insts[g]['conf'] for g in m), pred_mask=mask))
    return out


def _stitch_numpy(per_tile, base, insts, labels, tiles, n_points, thr, measure, min_shared, drop):
    ids_of = [_host(p).astype(np.int64) for p in tiles.point_ids]
    core_tile = _host(tiles.core_tile)
    rows = [M.packed_rows(ti, ids_of[t].size) if ti else None for t, ti in enumerate(per_tile)]
    edges = []
    for a, b in tiles.neighbours():
        if rows[a] is None or rows[b] is None:
            continue
        pos_a, pos_b = ST.tile_shared_numpy(ids_of[a], ids_of[b])
        if pos_a.size == 0:
            continue
        sa = RS.mask_bits_gather_numpy(rows[a], ids_of[a].size, pos_a)
        sb = RS.mask_bits_gather_numpy(rows[b], ids_of[b].size, pos_b)
        la, lb = labels[base[a]:base[a + 1]], labels[base[b]:base[b + 1]]
        link = ST.mask_cross_links_numpy(sa, sb, pos_a.size, la, lb, thr, measure, min_shared)[0]
        edges += [(base[a] + int(i), base[b] + int(j)) for i, j in zip(*np.nonzero(link))]
    n_total = len(insts)
    comp = ST.stitch_components_numpy(ST.adjacency_from_edges(edges, n_total), n_total)
    ids, cnt, core_cnt = [], [], []
    for t, r in enumerate(rows):
        if r is None:
            continue
        i, c, k = ST.mask_bits_ids_numpy(r, ids_of[t].size, ids_of[t], core_tile[ids_of[t]] == t)
        ids.append(i), cnt.append(c), core_cnt.append(k)
    cnt = np.concatenate(cnt) if cnt else np.zeros(0, np.int32)
    core_cnt = np.concatenate(core_cnt) if core_cnt else np.zeros(0, np.int32)
    objects, key = _objects(comp, core_cnt, insts, drop)
    ids = np.concatenate(ids) if ids else np.zeros(0, np.int32)
    starts, ends, bounds = ST.stitch_union_numpy(ids, np.repeat(key, cnt), len(objects), n_points)
    return _merged(objects, insts, M.rle_dicts_from_runs_numpy(starts, ends, bounds, n_points))


def _stitch_device(per_tile, base, insts, labels, tiles, n_points, thr, measure, min_shared, drop):
    import torch
    dev = tiles.core_tile.device if tiles.is_cuda else torch.device('cuda', torch.cuda.current_device())
    n_total = len(insts)
    if not ST.stitch_supported(n_total, 0, n_points):
        raise _OutOfRange(f'{n_total} tile instances over {n_points} points')
    with torch.cuda.device(dev):
        points = torch.as_tensor(tiles.tile_points).to(dev, torch.int32)
        core_tile = torch.as_tensor(tiles.core_tile).to(dev, torch.int32)
        off = tiles.offsets
        ids_of = [points[off[t]:off[t + 1]] for t in range(len(tiles))]
        d_labels = torch.from_numpy(labels).to(dev)
        bits, checks = [], []
        for t, ti in enumerate(per_tile):
            b, check = M.rows_device(ti, off[t + 1] - off[t], dev) if ti else (None, None)
            bits.append(b)
            if check is not None:
                checks.append(check)
        # the points every pair of neighbouring tiles shares: all pairs, then ONE read-back of the counts
        pairs = [(a, b) for a, b in tiles.neighbours() if bits[a] is not None and bits[b] is not None]
        counts = torch.zeros(max(len(pairs), 1), dtype=torch.int32, device=dev)
        shared = [ST.tile_shared(ids_of[a], ids_of[b], counts[k:k + 1])[:2] for k, (a, b) in enumerate(pairs)]
        counts = counts.cpu().tolist()
        adj = torch.zeros((n_total, (n_total + 31) // 32), dtype=torch.int32, device=dev)
        for (a, b), (pos_a, pos_b), c in zip(pairs, shared, counts):
            if c == 0:
                continue
            sa = RS.mask_bits_gather(bits[a], off[a + 1] - off[a], pos_a[:c])
            sb = RS.mask_bits_gather(bits[b], off[b + 1] - off[b], pos_b[:c])
            ST.mask_cross_links(sa, sb, c, d_labels[base[a]:base[a + 1]], d_labels[base[b]:base[b + 1]], base[a], base[b],
                                n_total, thr, measure, min_shared, adj=adj)
        comp = ST.stitch_components(adj, n_total)
        cnt = torch.zeros(n_total, dtype=torch.int32, device=dev)
        core_cnt = torch.zeros(n_total, dtype=torch.int32, device=dev)
        for t, b in enumerate(bits):
            if b is not None:
                ST.mask_bits_ids_count(b, off[t + 1] - off[t], core_tile[ids_of[t].long()] == t,
                                       cnt[base[t]:base[t + 1]], core_cnt[base[t]:base[t + 1]])
        check = torch.stack(checks).any(0).int() if checks else torch.zeros(2, dtype=torch.int32, device=dev)
        back = torch.cat([comp, cnt, core_cnt, check]).cpu().numpy()      # the one small read-back
        comp, cnt, core_cnt = back[:n_total], back[n_total:2 * n_total], back[2 * n_total:3 * n_total]
        M.raise_bad_rle(back[3 * n_total], back[3 * n_total + 1])
        total = int(cnt.astype(np.int64).sum())
        if not ST.stitch_supported(n_total, total, n_points):
            raise _OutOfRange(f'{total} mask points')
        objects, key = _objects(comp, core_cnt, insts, drop)
        n_obj = len(objects)
        if n_obj == 0:
            return []
        row_off = np.zeros(n_total, np.int64)
        np.cumsum(cnt[:-1], out=row_off[1:])
        d_off, d_key = torch.from_numpy(row_off).to(dev), torch.from_numpy(key).to(dev)
        ids = torch.empty(total, dtype=torch.int32, device=dev)
        keys = torch.empty(total, dtype=torch.int32, device=dev)
        meta = torch.zeros(1, dtype=torch.int32, device=dev)
        for t, b in enumerate(bits):
            if b is not None:
                ST.mask_bits_ids_fill(b, off[t + 1] - off[t], ids_of[t], n_points, d_off[base[t]:base[t + 1]],
                                      d_key[base[t]:base[t + 1]], ids, keys, meta)
        starts, ends, bounds = ST.stitch_union(ids, keys, n_obj, n_points)
        masks, flag = M.rle_dicts_from_runs_device(starts, ends, bounds, n_obj, n_points, dev, extra=meta)
        if flag[0]:
            raise ValueError('stitch_results: a point id of the tiles outside the cloud')
    return _merged(objects, insts, masks)


def stitch_results(results, tiles, coords=None, gt=None, thr=0.5, measure='iou', min_shared=1, drop_margin_only=True,
                   backend='auto'):
    """-> a NEW result dict over the ``tiles.n_points`` points of the full cloud (see the module text).
    ``results``: one result dict of ``forward_test`` / ``ScanForward`` per tile of ``tiles`` (a ``TileSet``), in
    tile order; ``coords``: the full cloud's coordinates [N, 3]; ``gt``: dict of the full cloud's label arrays.
    ``panoptic_preds`` is dropped: its ids are per tile."""
    from ..ops.nms import _measure
    _measure(measure)
    chosen = ST.auto_backend(backend, 'stitch')
    if isinstance(results, LazyResults):
        results.resolve()
    results = list(results)
    for r in results:
        if isinstance(r, LazyResults):
            r.resolve()
    if len(results) != len(tiles):
        raise ValueError(f'{len(results)} results for {len(tiles)} tiles')
    n_points = tiles.n_points
    n_tile = [tiles.offsets[t + 1] - tiles.offsets[t] for t in range(len(tiles))]
    gt = gt or {}
    out = {}
    first = results[0] if results else {}
    for key, value in dict.items(first):
        if key in _FROM_CORE:
            out[key] = _from_core(results, key, tiles, n_tile)
        elif key in _DROPPED or key in M._FROM_GT or key in ('pred_instances', 'coords_float'):
            pass
        else:
            out[key] = value
    if coords is not None:
        out['coords_float'] = M.full_cloud_coords(coords, n_points, 'a cloud')
    M.take_from_gt(out, gt)
    if not any('pred_instances' in r for r in results):
        return out
    per_tile = [list(r['pred_instances']) if 'pred_instances' in r else [] for r in results]
    base = [0]
    for t, ti in enumerate(per_tile):
        if ti and M.mask_length(ti) != n_tile[t]:
            raise ValueError(f'pred_instances of tile {t}: masks of {M.mask_length(ti)} points, '
                             f'the tile has {n_tile[t]}')
        base.append(base[-1] + len(ti))
    insts = [inst for ti in per_tile for inst in ti]
    labels = np.array([int(inst['label_id']) for inst in insts], dtype=np.int64).astype(np.int32)
    args = (per_tile, base, insts, labels, tiles, n_points, float(thr), measure, int(min_shared), bool(drop_margin_only))
    if not insts:
        out['pred_instances'] = []
    elif chosen == 'device':
        try:
            out['pred_instances'] = _stitch_device(*args)
        except _OutOfRange as e:
            if backend != 'auto':
                from .. import _lib as L
                raise L.SoftGroupHipError(f'stitch_results: {e}: outside the supported range (at most '
                                          f'{ST.MAX_INSTANCES} tile instances, fewer than 2**31 mask points and points)')
            out['pred_instances'] = _stitch_numpy(*args)
        except M.UnsortedRuns:
            if backend != 'auto':
                raise
            out['pred_instances'] = _stitch_numpy(*args)
    else:
        out['pred_instances'] = _stitch_numpy(*args)
    return out
