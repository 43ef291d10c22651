"""Overlapping tiles of a large cloud and the join of the instances that straddle a cut (csrc/stitch.hip): tile
membership, the points two tiles share, rectangular mask intersections with the link decision, connected components
of the link graph, the set bits of tile rows as global ids and the union of ids as maximal runs.

The reference has none of these (dataset/stpls3d/prepare_data_inst_instance_stpls3d.py cuts blocks offline and every
block is evaluated as a scene of its own); the rules are this project's and are stated in include/softgroup_hip.h:

* core cell of a point, per axis: ``c = floor((float64(x) - o) / size)`` -- one subtraction, one division; a
  coordinate that is not finite or ``|c| >= 2**30`` raises ``ValueError``; tiles split x and y only;
* the tiles are the cells with at least one core point, numbered in ascending ``(cy, cx)`` order, at most 65 535;
* overlap (``margin > 0``), per axis: ``lo = o + float64(c) * size``, ``hi = o + float64(c + 1) * size``; the point
  also belongs on the side ``c - 1`` when ``float64(x) < lo + margin``, else on the side ``c + 1`` when
  ``float64(x) >= hi - margin``; the axes combine (1, 2 or 4 candidate cells) and a neighbouring cell that is not a
  tile receives nothing; a tile's point list is ascending;
* link of two instances of neighbouring tiles with equal labels: ``inter >= min_shared``, ``den > 0`` and
  ``float64(inter) / float64(den) > thr`` strictly, ``den = ca + cb - inter`` ('iou') or ``min(ca, cb)`` ('min'),
  the populations counted over the points both tiles hold;
* an object is a connected component, named by its smallest member; its mask is the union of its members' ids.

CUDA tensors take the HIP kernels, numpy arrays the ``*_numpy`` twins, which are the definition the device results
are held to byte for byte.
"""
import numpy as np

from ._args import _words, _xyz_device, _xyz_numpy, choose_backend
from .nms import _measure, _popcount

__all__ = ['auto_backend', 'tile_assign', 'tile_assign_numpy', 'tile_shared', 'tile_shared_numpy', 'mask_cross_links',
           'mask_cross_links_numpy', 'stitch_components', 'stitch_components_numpy', 'mask_bits_ids_count',
           'mask_bits_ids_fill', 'mask_bits_ids_numpy', 'stitch_union', 'stitch_union_numpy', 'stitch_supported',
           'MAX_TILES', 'MAX_INSTANCES', 'MAX_DEVICE_POINTS']

MAX_TILES = 65535
MAX_INSTANCES = 16384
MAX_DEVICE_POINTS = 2**29          # sg_tile_assign_*: 4 memberships per point in int32 entry numbers

# what backend='auto' means with a GPU present -- the single place to change.  Both follow
# profiles/stitch_bench.txt, where the device is ahead of numpy on both instance sets: 0.93 ms against 254 ms for
# tile_cloud, 27 - 38 ms against 2813 - 5851 ms for stitch_results (2.4 M points in 16 tiles; wall, MI355X).
_AUTO = {'tiles': 'device', 'stitch': 'device'}


def auto_backend(backend, what):
    """'device' or 'numpy' for one of the operations of ``_AUTO``"""
    return choose_backend(backend, _AUTO[what])


def _tile_params(size, margin, origin):
    size, margin = float(size), float(margin)
    if not (size > 0.0 and np.isfinite(size)):
        raise ValueError(f'tile size {size!r}: a finite number > 0')
    if not 0.0 <= margin <= size / 2:
        raise ValueError(f'margin {margin!r}: between 0 and size / 2')
    if origin is not None:
        origin = (float(origin[0]), float(origin[1]))
        if not (np.isfinite(origin[0]) and np.isfinite(origin[1])):
            raise ValueError(f'origin {origin!r}: two finite numbers')
    return size, margin, origin


_BAD_POINT = 'tile_cloud: a coordinate that is not finite, or a cell index at or beyond 2**30 (tile size too small)'
_TOO_MANY = f'tile_cloud: more than {MAX_TILES} tiles (tile size too small for the cloud)'


# ---- tiles -----------------------------------------------------------------------------------------------------------
def _side(x, o, c, size, margin):
    lo = o + c.astype(np.float64) * size
    hi = o + (c + 1).astype(np.float64) * size
    left = x < lo + margin
    right = ~left & (x >= hi - margin)
    return right.astype(np.int64) - left.astype(np.int64)


def tile_assign_numpy(xyz, size, margin, origin=None):
    """-> (cells int32 [T, 2] = (cx, cy), tile_off int64 [T + 1], tile_points int32, core_tile int32 [n],
    core_pos int32 [n], origin): ``np.unique`` of the biased cell keys, a ``searchsorted`` per neighbour and one
    ``lexsort`` of the (tile, point) pairs"""
    size, margin, origin = _tile_params(size, margin, origin)
    xyz = _xyz_numpy(xyz)
    n = xyz.shape[0]
    if not np.isfinite(xyz).all():
        raise ValueError(_BAD_POINT)
    xy = xyz[:, :2].astype(np.float64)
    if origin is None:
        origin = (float(xy[:, 0].min()), float(xy[:, 1].min())) if n else (0.0, 0.0)
    if n == 0:
        return (np.zeros((0, 2), np.int32), np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32),
                np.zeros(0, np.int32), origin)
    cf = np.stack([np.floor((xy[:, 0] - origin[0]) / size), np.floor((xy[:, 1] - origin[1]) / size)], 1)
    if not (np.abs(cf) < 2.0**30).all():
        raise ValueError(_BAD_POINT)
    c = cf.astype(np.int64)

    def key(cx, cy):
        return ((cy + 2**30).astype(np.uint64) << np.uint64(32)) | (cx + 2**30).astype(np.uint64)

    tiles, core_tile = np.unique(key(c[:, 0], c[:, 1]), return_inverse=True)       # ascending key = ascending (cy, cx)
    core_tile = core_tile.reshape(-1)
    n_tiles = tiles.size
    if n_tiles > MAX_TILES:
        raise ValueError(_TOO_MANY)
    cells = np.stack([(tiles & np.uint64(0xFFFFFFFF)).astype(np.int64) - 2**30,
                      (tiles >> np.uint64(32)).astype(np.int64) - 2**30], 1).astype(np.int32)
    idx = np.arange(n, dtype=np.int64)
    ent_tile, ent_point = [core_tile.astype(np.int64)], [idx]
    if margin > 0.0:
        dx = _side(xy[:, 0], origin[0], c[:, 0], size, margin)
        dy = _side(xy[:, 1], origin[1], c[:, 1], size, margin)
        for sel, ddx, ddy in ((dx != 0, dx, 0), (dy != 0, 0, dy), ((dx != 0) & (dy != 0), dx, dy)):
            k = key((c[:, 0] + ddx)[sel], (c[:, 1] + ddy)[sel])
            at = np.minimum(np.searchsorted(tiles, k), n_tiles - 1)
            hit = tiles[at] == k                                                    # (a cell that is no tile receives nothing)
            ent_tile.append(at[hit].astype(np.int64))
            ent_point.append(idx[sel][hit])
    ent_tile, ent_point = np.concatenate(ent_tile), np.concatenate(ent_point)
    order = np.lexsort((ent_point, ent_tile))
    ent_tile, ent_point = ent_tile[order], ent_point[order]
    tile_off = np.zeros(n_tiles + 1, np.int64)
    np.cumsum(np.bincount(ent_tile, minlength=n_tiles), out=tile_off[1:])
    core_pos = np.empty(n, np.int64)
    is_core = core_tile[ent_point] == ent_tile
    core_pos[ent_point[is_core]] = (np.arange(ent_tile.size) - tile_off[ent_tile])[is_core]
    return (cells, tile_off, ent_point.astype(np.int32), core_tile.astype(np.int32), core_pos.astype(np.int32), origin)


def tile_assign(xyz, size, margin, origin=None):
    """``sg_tile_assign_count`` + ``sg_tile_assign_fill`` on a CUDA tensor [n, 3] -> the tuple of
    ``tile_assign_numpy`` as CUDA tensors.  One read-back of (T, flags, total) between the passes, and one of the
    per-axis minimum when ``origin`` is None.  Other inputs: numpy."""
    import torch
    if not (torch.is_tensor(xyz) and xyz.is_cuda):
        return tile_assign_numpy(xyz, size, margin, origin)
    from .. import _lib as L
    size, margin, origin = _tile_params(size, margin, origin)
    xyz = _xyz_device(xyz)
    n, dev = xyz.size(0), xyz.device
    if n >= MAX_DEVICE_POINTS:
        raise L.SoftGroupHipError(f'tile_assign: {n} points: outside the supported range (n < 2**29)')
    lib = L.lib()
    with torch.cuda.device(dev):
        if origin is None:
            if n:
                lo = xyz[:, :2].amin(0).double().cpu().tolist()
                if not np.isfinite(lo).all():
                    raise ValueError(_BAD_POINT)
                origin = (float(lo[0]), float(lo[1]))
            else:
                origin = (0.0, 0.0)
        meta = torch.empty(4, dtype=torch.int32, device=dev)
        ws = L.workspace(lib.sg_tile_assign_workspace_bytes(n), dev)
        x = L.ptr(xyz) if n else None
        L.check(lib.sg_tile_assign_count(x, n, size, margin, origin[0], origin[1], L.ptr(meta), L.ptr(ws), ws.numel(),
                                         L.stream()), 'sg_tile_assign_count')
        n_tiles, flags, total, _ = meta.cpu().tolist()
        if flags & 1:
            raise ValueError(_BAD_POINT)
        if flags & 2:
            raise ValueError(_TOO_MANY)
        cells = torch.empty((n_tiles, 2), dtype=torch.int32, device=dev)
        tile_off = torch.empty(n_tiles + 1, dtype=torch.int64, device=dev)
        tile_points = torch.empty(total, dtype=torch.int32, device=dev)
        core_tile = torch.empty(n, dtype=torch.int32, device=dev)
        core_pos = torch.empty(n, dtype=torch.int32, device=dev)
        ws2 = L.workspace(lib.sg_tile_assign_fill_workspace_bytes(total), dev)
        L.check(lib.sg_tile_assign_fill(x, n, size, margin, origin[0], origin[1], n_tiles, total,
                                        L.ptr(cells) if n else None, L.ptr(tile_off), L.ptr(tile_points) if n else None,
                                        L.ptr(core_tile) if n else None, L.ptr(core_pos) if n else None, L.ptr(ws),
                                        ws.numel(), L.ptr(ws2), ws2.numel(), L.stream()), 'sg_tile_assign_fill')
    return cells, tile_off, tile_points, core_tile, core_pos, origin


# ---- shared points ---------------------------------------------------------------------------------------------------
def tile_shared_numpy(a, b):
    """positions (int32, ascending) in two strictly ascending lists of their common elements"""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    _, pos_a, pos_b = np.intersect1d(a, b, assume_unique=True, return_indices=True)
    return pos_a.astype(np.int32), pos_b.astype(np.int32)


def tile_shared(a, b, count_out=None):
    """``sg_tile_shared``: two strictly ascending CUDA int32 lists -> (pos_a, pos_b, count): buffers of
    ``min(len)`` entries whose first ``count`` (a device int32 [1], or ``count_out``, a one-element view the caller
    owns) are written.  Nothing synchronises.  Other inputs: numpy (exact-size arrays and an int)."""
    import torch
    if not (torch.is_tensor(a) and a.is_cuda):
        pos_a, pos_b = tile_shared_numpy(a.numpy() if torch.is_tensor(a) else a, b.numpy() if torch.is_tensor(b) else b)
        return pos_a, pos_b, pos_a.size
    from .. import _lib as L
    dev = a.device
    a = a.to(torch.int32).reshape(-1).contiguous()
    b = torch.as_tensor(b).to(dev, torch.int32).reshape(-1).contiguous()
    n_a, n_b = a.numel(), b.numel()
    lib = L.lib()
    with torch.cuda.device(dev):
        cap = max(min(n_a, n_b), 1)
        pos_a = torch.empty(cap, dtype=torch.int32, device=dev)
        pos_b = torch.empty(cap, dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev) if count_out is None else count_out
        ws = L.workspace(lib.sg_tile_shared_workspace_bytes(n_a), dev)
        L.check(lib.sg_tile_shared(L.ptr(a) if n_a else None, n_a, L.ptr(b) if n_b else None, n_b, L.ptr(pos_a),
                                   L.ptr(pos_b), L.ptr(count), L.ptr(ws), ws.numel(), L.stream()), 'sg_tile_shared')
    return pos_a, pos_b, count


# ---- links -----------------------------------------------------------------------------------------------------------
def _rows64(packed, n_bits):
    """packed rows (any integer dtype) -> uint64 rows with the bits at and beyond n_bits cleared"""
    packed = np.ascontiguousarray(packed)
    n = packed.shape[0]
    nbytes = (int(n_bits) + 7) // 8
    rows = np.zeros((n, (nbytes + 7) // 8 * 8), dtype=np.uint8)
    if nbytes:
        rows[:, :nbytes] = packed.view(np.uint8).reshape(n, -1)[:, :nbytes]
        if n_bits & 7:
            rows[:, nbytes - 1] &= (1 << (n_bits & 7)) - 1
    return rows.view(np.uint64).reshape(n, -1)


def link_rule(inter, ca, cb, thr=0.5, measure='iou', min_shared=1):
    """the decision on integer arrays (broadcast): -> bool"""
    meas = _measure(measure)
    inter, ca, cb = np.asarray(inter, np.int64), np.asarray(ca, np.int64), np.asarray(cb, np.int64)
    den = ca + cb - inter if meas == 0 else np.minimum(ca, cb) + 0 * inter
    inter = inter + 0 * den
    ok = (den > 0) & (inter >= int(min_shared))
    out = np.zeros(den.shape, dtype=bool)
    out[ok] = inter[ok].astype(np.float64) / den[ok].astype(np.float64) > float(thr)
    return out


def mask_cross_links_numpy(bits_a, bits_b, n_bits, labels_a=None, labels_b=None, thr=0.5, measure='iou', min_shared=1):
    """packed rows [n_a, >= ceil(n_bits / 8) bytes] against [n_b, ...] -> (link bool [n_a, n_b], inter int32
    [n_a, n_b], ca int32 [n_a], cb int32 [n_b]); without labels every pair is a candidate"""
    ra, rb = _rows64(bits_a, n_bits), _rows64(bits_b, n_bits)
    n_a, n_b = ra.shape[0], rb.shape[0]
    ca = _popcount(ra).sum(1, dtype=np.int64) if ra.size else np.zeros(n_a, np.int64)
    cb = _popcount(rb).sum(1, dtype=np.int64) if rb.size else np.zeros(n_b, np.int64)
    inter = np.zeros((n_a, n_b), np.int64)
    if ra.size and rb.size:
        for i in range(n_a):
            inter[i] = _popcount(rb & ra[i]).sum(1, dtype=np.int64)
    link = link_rule(inter, ca[:, None], cb[None, :], thr, measure, min_shared)
    if labels_a is not None:
        link &= np.asarray(labels_a).reshape(-1, 1) == np.asarray(labels_b).reshape(1, -1)
    return link, inter.astype(np.int32), ca.astype(np.int32), cb.astype(np.int32)


def mask_cross_links(bits_a, bits_b, n_bits, labels_a, labels_b, base_a, base_b, n_total, thr=0.5, measure='iou',
                     min_shared=1, adj=None, return_counts=False):
    """``sg_mask_cross_links`` on CUDA bit rows int32 [n_a, W] / [n_b, W] (W = ceil(n_bits / 32)): links are OR-ed
    into ``adj`` int32 [n_total, ceil(n_total / 32)] (created zeroed when None) -> adj, and with ``return_counts``
    (adj, inter [n_a, n_b], ca, cb).  Nothing synchronises."""
    import torch

    from .. import _lib as L
    meas = _measure(measure)
    n_bits, n_total = int(n_bits), int(n_total)
    w = _words(n_bits)
    for b in (bits_a, bits_b):
        if b.dim() != 2 or b.element_size() != 4 or b.is_floating_point() or b.size(1) != w:
            raise ValueError(f'bits: integer tensors [n, {w}] of 32-bit words')
    dev = bits_a.device
    bits_a, bits_b = bits_a.contiguous(), bits_b.contiguous()
    n_a, n_b = bits_a.size(0), bits_b.size(0)
    if n_total > MAX_INSTANCES:
        raise L.SoftGroupHipError(f'mask_cross_links: {n_total} instances: outside the supported range '
                                  f'(at most {MAX_INSTANCES})')
    labels_a = torch.as_tensor(labels_a).to(dev, torch.int32).reshape(-1).contiguous()
    labels_b = torch.as_tensor(labels_b).to(dev, torch.int32).reshape(-1).contiguous()
    if labels_a.numel() != n_a or labels_b.numel() != n_b:
        raise ValueError('labels: one entry per row')
    with torch.cuda.device(dev):
        if adj is None:
            adj = torch.zeros((n_total, _words(n_total)), dtype=torch.int32, device=dev)
        inter = torch.zeros((n_a, n_b), dtype=torch.int32, device=dev) if return_counts else None
        ca = torch.zeros(n_a, dtype=torch.int32, device=dev) if return_counts else None
        cb = torch.zeros(n_b, dtype=torch.int32, device=dev) if return_counts else None
        L.check(L.lib().sg_mask_cross_links(L.ptr(bits_a) if bits_a.numel() else None, n_a,
                                            L.ptr(bits_b) if bits_b.numel() else None, n_b, n_bits,
                                            L.ptr(labels_a) if n_a else None, L.ptr(labels_b) if n_b else None,
                                            int(base_a), int(base_b), n_total, float(thr), meas, int(min_shared),
                                            L.ptr(adj) if adj.numel() else None,
                                            L.ptr(inter) if return_counts and inter.numel() else None,
                                            L.ptr(ca) if return_counts and n_a else None,
                                            L.ptr(cb) if return_counts and n_b else None, L.stream()),
                'sg_mask_cross_links')
    return (adj, inter, ca, cb) if return_counts else adj


# ---- components ------------------------------------------------------------------------------------------------------
def adjacency_from_edges(edges, n_total):
    """symmetric packed adjacency uint32 [n_total, ceil(n_total / 32)] of a list of (g, h) pairs"""
    adj = np.zeros((n_total, _words(n_total)), dtype=np.uint32)
    for g, h in edges:
        adj[g, h >> 5] |= np.uint32(1 << (h & 31))
        adj[h, g >> 5] |= np.uint32(1 << (g & 31))
    return adj


def stitch_components_numpy(adj, n_total):
    """packed adjacency -> comp int32 [n_total]: the smallest member of every node's component (union-find with the
    smaller root kept)"""
    n_total = int(n_total)
    adj = np.ascontiguousarray(adj).view(np.uint32).reshape(n_total, -1) if n_total else np.zeros((0, 0), np.uint32)
    parent = list(range(n_total))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    if n_total:
        dense = np.unpackbits(adj.view(np.uint8), axis=1, bitorder='little')[:, :n_total]
        for g, h in zip(*np.nonzero(dense)):
            rg, rh = find(int(g)), find(int(h))
            if rg != rh:
                parent[max(rg, rh)] = min(rg, rh)
    return np.array([find(g) for g in range(n_total)], dtype=np.int32)


def stitch_components(adj, n_total):
    """``sg_stitch_components`` on a CUDA adjacency int32 [n_total, ceil(n_total / 32)] -> comp int32 [n_total]"""
    import torch
    if not (torch.is_tensor(adj) and adj.is_cuda):
        return stitch_components_numpy(adj.numpy() if torch.is_tensor(adj) else adj, n_total)
    from .. import _lib as L
    n_total = int(n_total)
    if n_total > MAX_INSTANCES:
        raise L.SoftGroupHipError(f'stitch_components: {n_total} instances: outside the supported range '
                                  f'(at most {MAX_INSTANCES})')
    if adj.numel() != n_total * _words(n_total) or adj.element_size() != 4:
        raise ValueError(f'adj: an integer tensor [{n_total}, {_words(n_total)}] of 32-bit words')
    adj = adj.contiguous()
    with torch.cuda.device(adj.device):
        comp = torch.empty(n_total, dtype=torch.int32, device=adj.device)
        L.check(L.lib().sg_stitch_components(L.ptr(adj) if n_total else None, n_total, L.ptr(comp) if n_total else None,
                                             L.stream()), 'sg_stitch_components')
    return comp


# ---- set bits as ids -------------------------------------------------------------------------------------------------
def mask_bits_ids_numpy(bits, n_bits, index_map, core=None):
    """packed rows -> (ids int32 (row after row, bit order), cnt int32 [n], core_cnt int32 [n])"""
    bits = np.ascontiguousarray(bits)
    n, n_bits = bits.shape[0], int(n_bits)
    index_map = np.asarray(index_map).reshape(-1)
    dense = np.unpackbits(bits.view(np.uint8).reshape(n, -1), axis=1, bitorder='little')[:, :n_bits].astype(bool) \
        if n_bits else np.zeros((n, 0), bool)
    rows, pos = np.nonzero(dense)
    cnt = np.bincount(rows, minlength=n).astype(np.int32)
    core_cnt = np.zeros(n, np.int32) if core is None else \
        np.bincount(rows, weights=(np.asarray(core).reshape(-1)[pos] != 0), minlength=n).astype(np.int32)
    return index_map[pos].astype(np.int32), cnt, core_cnt


def mask_bits_ids_count(bits, n_bits, core=None, cnt=None, core_cnt=None):
    """``sg_mask_bits_ids_count``: CUDA bit rows int32 [n, ceil(n_bits / 32)], ``core`` uint8 [n_bits] or None
    -> (cnt int32 [n], core_cnt int32 [n]); ``cnt`` / ``core_cnt``: views to write into instead"""
    import torch

    from .. import _lib as L
    n_bits = int(n_bits)
    if bits.dim() != 2 or bits.element_size() != 4 or bits.size(1) != _words(n_bits):
        raise ValueError(f'bits: an integer tensor [n, {_words(n_bits)}] of 32-bit words')
    dev, n = bits.device, bits.size(0)
    bits = bits.contiguous()
    if core is not None:
        core = core.to(dev, torch.uint8).reshape(-1).contiguous()
        if core.numel() != n_bits:
            raise ValueError(f'core: {n_bits} flags')
    with torch.cuda.device(dev):
        cnt = torch.empty(n, dtype=torch.int32, device=dev) if cnt is None else cnt
        core_cnt = torch.empty(n, dtype=torch.int32, device=dev) if core_cnt is None else core_cnt
        assert cnt.numel() == n and core_cnt.numel() == n and cnt.is_contiguous() and core_cnt.is_contiguous()
        L.check(L.lib().sg_mask_bits_ids_count(L.ptr(bits) if bits.numel() else None, n, n_bits,
                                               L.ptr(core) if core is not None and n_bits else None,
                                               L.ptr(cnt) if n else None, L.ptr(core_cnt) if n else None, L.stream()),
                'sg_mask_bits_ids_count')
    return cnt, core_cnt


def mask_bits_ids_fill(bits, n_bits, index_map, n_points, row_off, row_key, ids, keys, meta):
    """``sg_mask_bits_ids_fill``: the ids ``index_map[p]`` of the set bits p of every row, from ``row_off[k]`` on in
    ``ids`` (int32) with ``row_key[k]`` beside them in ``keys`` (int32 storage of the uint32 keys); ``meta``: a
    zeroed int32 [1] that collects the flag of a map value outside [0, n_points)"""
    import torch

    from .. import _lib as L
    n_bits = int(n_bits)
    dev, n = bits.device, bits.size(0)
    bits = bits.contiguous()
    index_map = index_map.to(dev, torch.int32).reshape(-1).contiguous()
    row_off = row_off.to(dev, torch.int64).contiguous()
    row_key = row_key.to(dev, torch.int32).contiguous()
    if index_map.numel() != n_bits or row_off.numel() != n or row_key.numel() != n or ids.numel() != keys.numel():
        raise ValueError('mask_bits_ids_fill: array sizes')
    with torch.cuda.device(dev):
        L.check(L.lib().sg_mask_bits_ids_fill(L.ptr(bits) if bits.numel() else None, n, n_bits,
                                              L.ptr(index_map) if n_bits else None, int(n_points),
                                              L.ptr(row_off) if n else None, L.ptr(row_key) if n else None,
                                              L.ptr(ids) if ids.numel() else None, L.ptr(keys) if ids.numel() else None,
                                              ids.numel(), L.ptr(meta), L.stream()), 'sg_mask_bits_ids_fill')


# ---- union -----------------------------------------------------------------------------------------------------------
def stitch_union_numpy(ids, keys, n_obj, n_points=None):
    """(id, object) pairs -> (starts int32, ends int32, bounds int64 [n_obj + 1]): per object the maximal runs of
    its distinct ids, 0-based, end exclusive, ascending; a key >= n_obj belongs to no object"""
    ids = np.asarray(ids).reshape(-1).astype(np.int64)
    keys = np.asarray(keys).reshape(-1).astype(np.int64) & 0xFFFFFFFF
    ok = keys < n_obj
    if n_points is not None:
        ok &= (ids >= 0) & (ids < n_points)
    pairs = np.unique(np.stack([keys[ok], ids[ok]], 1), axis=0) if ok.any() else np.zeros((0, 2), np.int64)
    k, v = pairs[:, 0], pairs[:, 1]
    head = np.ones(k.size, bool)
    head[1:] = (k[1:] != k[:-1]) | (v[1:] != v[:-1] + 1)
    tail = np.ones(k.size, bool)
    tail[:-1] = head[1:]
    bounds = np.zeros(n_obj + 1, np.int64)
    np.cumsum(np.bincount(k[head], minlength=n_obj), out=bounds[1:])
    return v[head].astype(np.int32), (v[tail] + 1).astype(np.int32), bounds


def stitch_supported(n_inst, total, n_points):
    """whether ``n_inst`` tile instances with ``total`` mask points over ``n_points`` points are inside the device's
    range (G <= 16384, total < 2**31, N < 2**31) -- the rule of ``sg_stitch_union_workspace_bytes``, asked of it"""
    from .. import _lib as L
    if not (0 <= int(n_inst) <= 2**31 - 1 and 0 <= int(total) < 2**63 and 0 <= int(n_points) < 2**63):
        return False
    return L.lib().sg_stitch_union_workspace_bytes(int(total), int(n_inst), int(n_points)) != 0


def stitch_union(ids, keys, n_obj, n_points):
    """``sg_stitch_union_count`` + ``_fill``: CUDA int32 ids / keys -> (starts int32, ends int32, bounds int64
    [n_obj + 1]) on the device, what ``sg_rle_format_device`` takes.  One read-back (the run total) between the
    passes.  Other inputs: numpy."""
    import torch
    if not (torch.is_tensor(ids) and ids.is_cuda):
        return stitch_union_numpy(ids, keys, n_obj, n_points)
    from .. import _lib as L
    dev = ids.device
    ids = ids.to(torch.int32).reshape(-1).contiguous()
    keys = keys.to(dev).reshape(-1).contiguous()
    if keys.element_size() != 4 or keys.numel() != ids.numel():
        raise ValueError('keys: one 32-bit word per id')
    total, n_obj, n_points = ids.numel(), int(n_obj), int(n_points)
    lib = L.lib()
    with torch.cuda.device(dev):
        nb = lib.sg_stitch_union_workspace_bytes(total, n_obj, n_points)
        if nb == 0:
            raise L.SoftGroupHipError(f'stitch_union: {total} ids, {n_obj} objects, {n_points} points: outside the '
                                      f'supported range (< 2**31, <= {MAX_INSTANCES}, < 2**31)')
        ws = L.workspace(nb, dev)
        bounds = torch.empty(n_obj + 1, dtype=torch.int64, device=dev)
        L.check(lib.sg_stitch_union_count(L.ptr(ids) if total else None, L.ptr(keys) if total else None, total, n_obj,
                                          n_points, L.ptr(bounds), L.ptr(ws), ws.numel(), L.stream()),
                'sg_stitch_union_count')
        runs = int(bounds[n_obj].item())
        starts = torch.empty(max(runs, 1), dtype=torch.int32, device=dev)
        ends = torch.empty(max(runs, 1), dtype=torch.int32, device=dev)
        L.check(lib.sg_stitch_union_fill(total, n_obj, n_points, L.ptr(ws), ws.numel(), L.ptr(starts), L.ptr(ends), runs,
                                         L.stream()), 'sg_stitch_union_fill')
    return starts[:runs], ends[:runs], bounds
