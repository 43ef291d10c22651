"""``tile_cloud`` and ``stitch_results``: the numpy twins of ``softgroup_amd.ops.stitch`` against plain-loop
restatements written HERE -- Python floats, dicts keyed by the cell tuple, sets of point ids, a breadth-first walk.
Equality everywhere, no tolerances.  tests/test_stitch_gpu.py holds the HIP kernels of csrc/stitch.hip to the same
references on the same inputs.  (None of these modules exists before this feature.)"""
import copy
import functools
import math

import numpy as np
import pytest
import torch

from softgroup_amd import synthetic
from softgroup_amd.data import TileSet, apply_sample, tile_cloud
from softgroup_amd.ops import stitch as ST
from softgroup_amd.util import rle_decode, rle_encode, stitch_results

EDGE_N = [0, 1, 63, 64, 65]


# ---- tiles ------------------------------------------------------------------------------------------------------------
def brute_tiles(xyz, size, margin, origin):
    """-> (cells [(cx, cy)], lists of point indices per tile, core_tile, core_pos, candidate cells per point): Python
    floats and a dict"""
    ox, oy = origin
    core, sides = [], []
    for x, y, _ in xyz.tolist():                      # (float32 values as Python doubles)
        c, d = [], []
        for v, o in ((x, ox), (y, oy)):
            k = math.floor((v - o) / size)
            side = 0
            if margin > 0:
                lo = o + float(k) * size
                hi = o + float(k + 1) * size
                if v < lo + margin:
                    side = -1
                elif v >= hi - margin:
                    side = 1
            c.append(k), d.append(side)
        core.append((c[0], c[1])), sides.append((d[0], d[1]))
    cells = sorted(set(core), key=lambda c: (c[1], c[0]))
    number = {c: t for t, c in enumerate(cells)}
    lists, n_cand = [[] for _ in cells], []
    for i, ((cx, cy), (dx, dy)) in enumerate(zip(core, sides)):
        cand = [(cx, cy)]
        if dx:
            cand.append((cx + dx, cy))
        if dy:
            cand.append((cx, cy + dy))
        if dx and dy:
            cand.append((cx + dx, cy + dy))
        n_cand.append(len(cand))
        for c in cand:
            if c in number:
                lists[number[c]].append(i)
    core_tile = [number[c] for c in core]
    core_pos = [lists[t].index(i) for i, t in enumerate(core_tile)] if len(core) < 20000 else None
    return cells, lists, core_tile, core_pos, n_cand


@functools.lru_cache(maxsize=None)
def tile_cases():
    """name -> (xyz, size, margin, origin); the clouds are read-only"""
    rng = np.random.default_rng(11)
    out = {}
    # a 1/64 lattice: hundreds of points exactly on tile faces and on hi - margin (all representable)
    x = np.round((rng.random((4000, 3)) * [5.0, 3.0, 2.0] - [2.0, 1.0, 0.0]) * 64) / 64
    x[:300, 0] = np.round(x[:300, 0] * 2) / 2                  # on faces of size 0.5
    x[300:600, 1] = np.round(x[300:600, 1] * 2) / 2 + 0.375      # on hi - margin for margin 0.125
    out['lattice'] = (x.astype(np.float32), 0.5, 0.125, (0.0, 0.0))
    out['lattice_no_margin'] = (out['lattice'][0], 0.5, 0.0, (0.0, 0.0))
    out['lattice_half'] = (out['lattice'][0], 0.5, 0.25, (0.0, 0.0))
    out['lattice_auto_origin'] = (out['lattice'][0], 0.5, 0.125, None)
    # size 0.1: its multiples are not representable; points on k * 0.1 and on k * 0.1 - margin as float32 and float64
    y = rng.random((5000, 3)) * [1.5, 1.2, 1.0] - [0.3, 0.2, 0.0]
    k = rng.integers(-3, 12, 5000)
    y[:400, 0] = k[:400] * 0.1
    y[400:800, 1] = k[400:800] * 0.1 - 0.02
    y[800:1000, 0] = (k[800:1000] * np.float64(0.1)).astype(np.float32)
    out['tenth'] = (y.astype(np.float32), 0.1, 0.02, (0.0, 0.0))
    out['tenth_half'] = (out['tenth'][0], 0.1, 0.05, (0.0, 0.0))
    out['full_grid'] = ((rng.random((4000, 3)) * [2.0, 1.5, 1.0] + [0.0, 0.0, 0.0]).astype(np.float32), 0.5, 0.125, (0.0, 0.0))
    out['single_tile'] = ((rng.random((3000, 3)) * 0.9 + 0.05).astype(np.float32), 1.0, 0.25, (0.0, 0.0))
    # holes: two clusters and a thin bridge; points in the margin next to cells that are no tiles
    z = np.concatenate([rng.random((1500, 3)) * [1.0, 1.0, 1.0], rng.random((1500, 3)) * [1.0, 1.0, 1.0] + [3.0, 2.0, 0.0],
                        np.stack([np.linspace(1.0, 3.0, 200), np.full(200, 0.49), np.zeros(200)], 1)])
    out['holes'] = (z.astype(np.float32), 0.5, 0.1, (0.0, 0.0))
    for v in out.values():
        v[0].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tile_reference(name):
    xyz, size, margin, origin = tile_cases()[name]
    if origin is None:
        origin = (float(xyz[:, 0].astype(np.float64).min()), float(xyz[:, 1].astype(np.float64).min()))
    return brute_tiles(xyz, size, margin, origin)


def edge_tile_cloud(n):
    return tile_cases()['lattice'][0][1000:1000 + n].copy()


def check_tiles(ts, ref, n, full_grid=False):
    """ascending lists, consistent core positions, 1, 2 or 4 candidate cells per point and as many tiles (fewer only
    where a candidate cell is no tile, never on a full grid), equal to the brute force"""
    cells, lists, core_tile, core_pos, n_cand = ref
    host = lambda a: a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)      # noqa: E731
    assert isinstance(ts, TileSet) and ts.n_points == n and len(ts) == len(cells)
    assert host(ts.cells).tolist() == [list(c) for c in cells]
    mult = np.zeros(n, np.int64)
    for ids, want in zip(ts.point_ids, lists):
        ids = host(ids)
        assert ids.dtype == np.int64 and (np.diff(ids) > 0).all()
        assert ids.tolist() == want
        mult[ids] += 1
    assert set(n_cand) <= {1, 2, 4} and (mult <= np.array(n_cand, np.int64)).all() and (n == 0 or mult.min() >= 1)
    if full_grid:
        assert set(np.unique(mult).tolist()) <= {1, 2, 4}
    assert host(ts.core_tile).tolist() == core_tile
    if core_pos is not None:
        assert host(ts.core_pos).tolist() == core_pos
    for i in range(0, n, max(n // 50, 1)):
        assert int(host(ts.point_ids[core_tile[i]])[int(host(ts.core_pos)[i])]) == i
    want_pairs = sorted((a, b) for a in range(len(cells)) for b in range(a + 1, len(cells))
                        if max(abs(cells[a][0] - cells[b][0]), abs(cells[a][1] - cells[b][1])) <= 1)
    assert ts.neighbours() == want_pairs


BAD_TILE_CLOUDS = {      # (row 1 is the invalid point) -> (xyz, size)
    'nan': (np.array([[0, 0, 0], [1, np.nan, 0], [2, 2, 2]], np.float32), 1.0),
    'nan_z': (np.array([[0, 0, 0], [1, 1, np.nan], [2, 2, 2]], np.float32), 1.0),
    'inf': (np.array([[0, 0, 0], [-np.inf, 2, 2], [1, 1, 1]], np.float32), 1.0),
    'range': (np.array([[0, 0, 0], [1e7, 1, 1], [2, 2, 2]], np.float32), 1e-3),
}


def too_many_tiles_cloud():
    g = np.arange(257, dtype=np.float32)
    x, y = np.meshgrid(g, g)
    return np.stack([x.ravel() + 0.5, y.ravel() + 0.5, np.zeros(257 * 257, np.float32)], 1)      # 66 049 cells


@pytest.mark.parametrize('name', sorted(tile_cases()))
def test_tile_cloud_numpy_equals_plain_loop(name):
    xyz, size, margin, origin = tile_cases()[name]
    ts = tile_cloud(xyz, size=size, margin=margin, origin=origin, backend='numpy')
    check_tiles(ts, tile_reference(name), xyz.shape[0], full_grid=name in ('full_grid', 'single_tile'))
    mult = np.bincount(np.concatenate(ts.point_ids), minlength=xyz.shape[0])
    if margin == 0:
        assert (mult == 1).all()
    else:
        assert (mult == 2).any() and (mult == 4).any() or name == 'single_tile'
    if name == 'single_tile':
        assert len(ts) == 1 and (mult == 1).all()
    if name == 'full_grid':                 # interior corners are in 4 tiles; the cloud's own border has no neighbour
        assert len(ts) == 12 and (mult == 4).sum() > 100 and (mult == 3).sum() == 0
    if name == 'holes':                     # the bridge's points lie in the margin of cells (y = 1) that hold no core point
        assert ((1 <= xyz[:, 0]) & (xyz[:, 0] <= 3) & (xyz[:, 1] == np.float32(0.49))).sum() == 200
        cells = set(map(tuple, ts.cells.tolist()))
        assert (3, 1) not in cells and (3, 0) in cells
    if name == 'lattice':
        on_face = (np.mod(xyz[:, :2].astype(np.float64), 0.5) == 0).any(1).sum()
        assert on_face >= 300


@pytest.mark.parametrize('n', EDGE_N)
def test_tile_cloud_numpy_edge_sizes(n):
    x = edge_tile_cloud(n)
    ts = tile_cloud(x, size=0.5, margin=0.125, origin=(0.0, 0.0), backend='numpy')
    check_tiles(ts, brute_tiles(x, 0.5, 0.125, (0.0, 0.0)), n)


@pytest.mark.parametrize('name', sorted(BAD_TILE_CLOUDS))
def test_tile_cloud_numpy_rejects_invalid_points(name):
    x, size = BAD_TILE_CLOUDS[name]
    with pytest.raises(ValueError):
        tile_cloud(x, size=size, margin=0.0, origin=(0.0, 0.0), backend='numpy')


def test_tile_cloud_numpy_rejects_bad_parameters_and_too_many_tiles():
    x = tile_cases()['lattice'][0][:10]
    for kw in (dict(size=0.0), dict(size=np.inf), dict(size=1.0, margin=0.6), dict(size=1.0, margin=-0.1),
               dict(size=1.0, margin=0.1, origin=(np.nan, 0.0))):
        with pytest.raises(ValueError):
            tile_cloud(x, backend='numpy', **kw)
    with pytest.raises(ValueError):
        tile_cloud(x, size=1.0, margin=0.1, backend='gpu')
    with pytest.raises(ValueError, match='65535'):
        tile_cloud(too_many_tiles_cloud(), size=1.0, margin=0.0, origin=(0.0, 0.0), backend='numpy')
    ok = tile_cloud(too_many_tiles_cloud()[:65535], size=1.0, margin=0.0, origin=(0.0, 0.0), backend='numpy')
    assert len(ok) == 65535


def test_tile_cloud_keeps_the_input_kind_and_feeds_apply_sample():
    xyz = tile_cases()['lattice'][0]
    ts = tile_cloud(torch.from_numpy(xyz.copy()), size=0.5, margin=0.125, origin=(0.0, 0.0), backend='numpy')
    assert torch.is_tensor(ts.core_tile) and ts.point_ids[0].dtype == torch.int64
    check_tiles(ts, tile_reference('lattice'), xyz.shape[0])
    ts = tile_cloud(xyz, size=0.5, margin=0.125, origin=(0.0, 0.0), backend='numpy')
    sem = np.arange(xyz.shape[0])
    a, b, c, d = apply_sample(ts.point_ids[3], xyz, xyz, sem, sem)
    assert np.array_equal(c, ts.point_ids[3]) and np.array_equal(a, xyz[ts.point_ids[3]])


# ---- shared points ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shared_cases():
    rng = np.random.default_rng(5)
    pool = np.sort(rng.choice(40000, 18000, replace=False)).astype(np.int32)
    a, b = pool[rng.random(18000) < 0.5], pool[rng.random(18000) < 0.5]
    return {'empty_a': (pool[:0], pool[:9]), 'empty_b': (pool[:9], pool[:0]), 'one_hit': (pool[5:6], pool[:65]),
            'one_miss': (pool[70:71], pool[:65]), 'sixty_five': (pool[:65], pool[30:95]), 'large': (a, b),
            'disjoint': (pool[0::2][:3000], pool[1::2][:3000]), 'identical': (a, a.copy())}


def brute_shared(a, b):
    where = {int(v): j for j, v in enumerate(b.tolist())}
    hits = [(i, where[int(v)]) for i, v in enumerate(a.tolist()) if int(v) in where]
    return [h[0] for h in hits], [h[1] for h in hits]


@pytest.mark.parametrize('name', sorted(shared_cases()))
def test_tile_shared_numpy(name):
    a, b = shared_cases()[name]
    pos_a, pos_b = ST.tile_shared_numpy(a, b)
    want = brute_shared(a, b)
    assert pos_a.dtype == pos_b.dtype == np.int32 and pos_a.tolist() == want[0] and pos_b.tolist() == want[1]
    if name == 'large':
        assert 8000 <= a.size <= 10000 and 3000 < pos_a.size < 6000


# ---- links ------------------------------------------------------------------------------------------------------------
def packed_rows(dense):
    n, n_bits = dense.shape
    out = np.zeros((n, (n_bits + 31) // 32 * 4), np.uint8)
    if n_bits:
        p = np.packbits(dense, axis=1, bitorder='little')
        out[:, :p.shape[1]] = p
    return out


LINK_BITS = [1, 31, 32, 33, 2047, 2049, 20001]
LINK_SHAPES = [(1, 1), (3, 5), (4, 4), (5, 37), (37, 3)]


@functools.lru_cache(maxsize=None)
def link_case(n_bits, n_a, n_b):
    """dense masks with heavy overlaps, labels from {1, 2}, and packed rows with garbage beyond n_bits"""
    rng = np.random.default_rng(n_bits * 1000 + n_a * 50 + n_b)
    a = rng.random((n_a, n_bits)) < 0.4
    b = rng.random((n_b, n_bits)) < 0.4
    for j in range(min(n_a, n_b)):          # near copies: pairs on both sides of the threshold
        b[j] = a[j] ^ (rng.random(n_bits) < 0.15 * (j % 4))
    if n_a > 2:
        a[2] = False                        # an empty row: den == 0 against an empty partner
    if n_b > 2:
        b[2] = False
    la, lb = rng.integers(1, 3, n_a).astype(np.int32), rng.integers(1, 3, n_b).astype(np.int32)
    pa, pb = packed_rows(a), packed_rows(b)
    if n_bits & 31:
        garbage = np.uint8((0xFF << (n_bits & 7)) & 0xFF) if n_bits & 7 else np.uint8(0)
        for p in (pa, pb):
            p[:, (n_bits + 7) // 8:] = 0xA5
            p[:, (n_bits - 1) // 8] |= garbage
    return a, b, la, lb, pa, pb


def brute_links(a, b, la, lb, thr, measure, min_shared):
    link = np.zeros((a.shape[0], b.shape[0]), bool)
    inter = np.zeros((a.shape[0], b.shape[0]), np.int32)
    for i in range(a.shape[0]):
        sa = set(np.flatnonzero(a[i]).tolist())
        for j in range(b.shape[0]):
            sb = set(np.flatnonzero(b[j]).tolist())
            it = len(sa & sb)
            inter[i, j] = it
            den = len(sa) + len(sb) - it if measure == 'iou' else min(len(sa), len(sb))
            link[i, j] = la[i] == lb[j] and it >= min_shared and den > 0 and it / den > thr
    return link, inter


def test_link_rule_at_the_threshold():
    assert not ST.link_rule(1, 1, 2, thr=0.5, measure='iou')              # inter 1, den 2: exactly 0.5 is not over it
    assert ST.link_rule(2, 2, 3, thr=0.5, measure='iou')
    assert ST.link_rule(1, 1, 2, thr=0.5, measure='min')                  # den = min = 1
    assert not ST.link_rule(1, 2, 2, thr=0.5, measure='min')
    assert not ST.link_rule(0, 0, 0, thr=-1.0)                            # den == 0
    assert ST.link_rule(0, 1, 1, thr=-1.0, min_shared=0) and not ST.link_rule(0, 1, 1, thr=-1.0, min_shared=1)
    assert ST.link_rule(3, 3, 3, thr=0.5, min_shared=3) and not ST.link_rule(3, 3, 3, thr=0.5, min_shared=4)
    with pytest.raises(ValueError):
        ST.link_rule(1, 1, 1, measure='dice')


@pytest.mark.parametrize('measure', ['iou', 'min'])
@pytest.mark.parametrize('n_bits,shape', [(33, (3, 5)), (2049, (5, 37)), (31, (4, 4)), (1, (1, 1))])
def test_mask_cross_links_numpy_equals_sets(n_bits, shape, measure):
    a, b, la, lb, pa, pb = link_case(n_bits, *shape)
    n_links = []
    for min_shared in (1, 3, n_bits + 1):
        link, inter, ca, cb = ST.mask_cross_links_numpy(pa, pb, n_bits, la, lb, 0.5, measure, min_shared)
        want, want_inter = brute_links(a, b, la, lb, 0.5, measure, min_shared)
        assert np.array_equal(link, want) and np.array_equal(inter, want_inter)
        assert np.array_equal(ca, a.sum(1)) and np.array_equal(cb, b.sum(1))
        n_links.append(int(want.sum()))
    assert n_links[-1] == 0
    if n_bits == 2049:
        assert n_links[0] >= 1 and (la[:, None] != lb[None, :]).any()
        unlabelled = ST.mask_cross_links_numpy(pa, pb, n_bits, None, None, 0.5, measure, 1)[0]
        assert unlabelled.sum() > n_links[0]                  # pairs that only their labels keep apart


# ---- components -------------------------------------------------------------------------------------------------------
def path_edges(n):
    """a path whose smallest label sits at one end and whose numbering zigzags, so a label travels the whole path"""
    order = [0] + [n - 1 - k // 2 if k % 2 == 0 else 1 + k // 2 for k in range(n - 1)]
    return list(zip(order[:-1], order[1:]))


@functools.lru_cache(maxsize=None)
def graph_cases():
    rng = np.random.default_rng(9)
    rand = [tuple(e) for e in rng.integers(0, 500, (260, 2)).tolist() if e[0] != e[1]]
    return {'path300': (300, path_edges(300)), 'path1025': (1025, path_edges(1025)),
            'star': (70, [(69, k) for k in range(69)]), 'same_tile_through_third': (5, [(1, 4), (3, 4)]),
            'one': (1, []), 'thirty_three': (33, [(32, 0), (31, 1), (5, 6), (6, 7)]), 'none': (40, []),
            'random500': (500, rand)}


def brute_components(n, edges):
    nbr = [[] for _ in range(n)]
    for g, h in edges:
        nbr[g].append(h), nbr[h].append(g)
    comp = [-1] * n
    for s in range(n):
        if comp[s] >= 0:
            continue
        comp[s], todo = s, [s]
        while todo:
            for h in nbr[todo.pop()]:
                if comp[h] < 0:
                    comp[h] = s
                    todo.append(h)
    return comp


@pytest.mark.parametrize('name', sorted(graph_cases()))
def test_stitch_components_numpy(name):
    n, edges = graph_cases()[name]
    comp = ST.stitch_components_numpy(ST.adjacency_from_edges(edges, n), n)
    assert comp.dtype == np.int32 and comp.tolist() == brute_components(n, edges)
    if name.startswith('path'):
        assert not comp.any() and len(edges) == n - 1
    if name == 'same_tile_through_third':
        assert comp.tolist() == [0, 1, 2, 1, 1]


# ---- union ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def union_cases():
    """name -> (n_points, n_obj, [(object key, ids)])  (key -1 / >= n_obj: no object)"""
    rng = np.random.default_rng(21)
    big = [(int(rng.integers(0, 9)) - 1, np.sort(rng.choice(70001, int(rng.integers(1, 4000)), replace=False)))
           for _ in range(40)]
    return {
        'shared_ids': (100, 1, [(0, [3, 4, 5, 9]), (0, [4, 5, 6, 9])]),
        'adjacent_members': (100, 2, [(0, [10, 12]), (1, [11]), (0, [11, 13]), (1, [50])]),
        'ends': (77, 1, [(0, [0, 1]), (0, [76])]),
        'odd_length': (33, 2, [(1, [31, 32]), (0, [0, 32])]),
        'empty_object': (64, 3, [(0, [1]), (2, [5, 6])]),
        'dropped_member': (64, 1, [(0, [1, 2]), (-1, [3, 4]), (7, [9])]),
        'nothing': (64, 2, []),
        'large': (70001, 8, big),
    }


def union_inputs(case):
    n_points, n_obj, members = case
    ids = np.concatenate([np.asarray(m[1], np.int32) for m in members]) if members else np.zeros(0, np.int32)
    keys = np.concatenate([np.full(len(m[1]), m[0], np.int32) for m in members]) if members else np.zeros(0, np.int32)
    return ids, keys


def brute_union(case):
    n_points, n_obj, members = case
    out = []
    for o in range(n_obj):
        dense = np.zeros(n_points, np.uint8)
        for k, ids in members:
            if k == o:
                dense[np.asarray(ids, np.int64)] = 1
        out.append(rle_encode(dense))
    return out


def runs_to_rle(n_points, starts, ends, bounds):
    from softgroup_amd.util import rle_encode_runs
    return [rle_encode_runs(n_points, starts[bounds[o]:bounds[o + 1]],
                            ends[bounds[o]:bounds[o + 1]].astype(np.int64) - starts[bounds[o]:bounds[o + 1]])
            for o in range(len(bounds) - 1)]


@pytest.mark.parametrize('name', sorted(union_cases()))
def test_stitch_union_numpy_equals_rle_of_the_dense_union(name):
    case = union_cases()[name]
    ids, keys = union_inputs(case)
    starts, ends, bounds = ST.stitch_union_numpy(ids, keys, case[1], case[0])
    assert starts.dtype == ends.dtype == np.int32 and bounds.dtype == np.int64
    assert runs_to_rle(case[0], starts, ends, bounds) == brute_union(case)
    if name == 'adjacent_members':
        assert starts.tolist() == [10, 11, 50] and ends.tolist() == [14, 12, 51]


def test_mask_bits_ids_numpy():
    rng = np.random.default_rng(2)
    dense = rng.random((7, 1001)) < 0.3
    dense[4] = False
    index_map = np.sort(rng.choice(5000, 1001, replace=False)).astype(np.int32)
    core = rng.random(1001) < 0.5
    ids, cnt, core_cnt = ST.mask_bits_ids_numpy(packed_rows(dense), 1001, index_map, core)
    assert ids.tolist() == [int(index_map[p]) for r in range(7) for p in np.flatnonzero(dense[r])]
    assert cnt.tolist() == dense.sum(1).tolist() and core_cnt.tolist() == (dense & core).sum(1).tolist()


# ---- end to end, no model --------------------------------------------------------------------------------------------
E2E_CASES = [(1, 30000, 2.0, 0.5), (1, 30000, 2.0, 0.25), (4, 20000, 1.5, 0.3)]
E2E_COUNTS = {E2E_CASES[0]: (12, 42), E2E_CASES[1]: (12, 38), E2E_CASES[2]: (20, 48)}      # (tiles, tile instances)


def fake_scan(ids, inst, sem, tile, thin=None):
    """the result of a perfect scan of one tile: for every labelled object with a point in the tile exactly that
    object's points in the tile; label 2 + k % 3, distinct scores"""
    local = inst[ids]
    insts = []
    for k in np.unique(local[local >= 0]).tolist():
        mask = local == k
        if thin is not None:
            mask &= thin.random(mask.size) >= 0.1
        insts.append(dict(scan_id='scene', obj=k, label_id=2 + k % 3, conf=0.3 + 0.01 * k + 0.0007 * tile,
                          pred_mask=rle_encode(mask.astype(np.uint8))))
    rng = np.random.default_rng(tile)
    return dict(scan_id='scene', semantic_preds=sem[ids] + 100 * tile, offset_preds=rng.random((ids.size, 3), np.float32),
                panoptic_preds=np.arange(ids.size, dtype=np.uint32), coords_float=np.zeros((ids.size, 3), np.float32),
                semantic_labels=sem[ids], instance_labels=local, pred_instances=insts)


@functools.lru_cache(maxsize=None)
def e2e_case(seed, n, size, margin, thinned=False):
    xyz, _, inst = synthetic.scene_s2(seed=seed, n=n)
    sem = np.where(inst >= 0, 2 + inst % 3, 0).astype(np.int64)
    tiles = tile_cloud(xyz, size=size, margin=margin, origin=(-0.5, -0.5), backend='numpy')
    thin = np.random.default_rng(77) if thinned else None
    results = [fake_scan(ids, inst, sem, t, thin) for t, ids in enumerate(tiles.point_ids)]
    return xyz, inst, sem, tiles, results


def check_e2e(out, case, thinned=False):
    xyz, inst, sem, tiles, results = case
    n = xyz.shape[0]
    flat = [i for r in results for i in r['pred_instances']]
    assert len(flat) >= 30, 'the merge must be exercised'
    got = out['pred_instances']
    assert len(got) == 12
    first_of, best = {}, {}
    for g, i in enumerate(flat):
        k = i['obj']                                          # the object the fake scan made it from
        first_of.setdefault(k, g)
        best[k] = max(best.get(k, 0.0), i['conf'])
    order = sorted(first_of, key=first_of.get)
    for k, g in zip(order, got):
        m = rle_decode(g['pred_mask']).astype(bool)
        assert g['pred_mask']['length'] == n and g['label_id'] == 2 + k % 3 and g['scan_id'] == 'scene'
        assert g['conf'] == best[k]
        if thinned:
            assert m.sum() > 0 and not (m & (inst != k)).any()
        else:
            assert np.array_equal(m, inst == k)
        assert g['pred_mask'] == rle_encode(m.astype(np.uint8))
    core_tile, core_pos = np.asarray(tiles.core_tile), np.asarray(tiles.core_pos)
    for key in ('semantic_preds', 'offset_preds'):
        for p in range(0, n, 97):
            assert np.array_equal(out[key][p], results[core_tile[p]][key][core_pos[p]])
    assert np.array_equal(out['semantic_preds'] % 100, sem) and (out['semantic_preds'] // 100 == core_tile).all()
    assert 'panoptic_preds' not in out and out['scan_id'] == 'scene'
    assert out['coords_float'] is xyz and out['semantic_labels'] is sem and 'instance_labels' not in out


@pytest.mark.parametrize('case', E2E_CASES)
def test_stitch_results_numpy_recovers_the_objects(case):
    data = e2e_case(*case)
    tiles, results = data[3], data[4]
    assert (len(tiles), sum(len(r['pred_instances']) for r in results)) == E2E_COUNTS[case]
    before = copy.deepcopy(results)
    out = stitch_results(results, tiles, coords=data[0], gt=dict(semantic_labels=data[2]), backend='numpy')
    check_e2e(out, data)
    for r, b in zip(results, before):                     # inputs not modified
        assert r.keys() == b.keys() and r['pred_instances'] == b['pred_instances']
        assert np.array_equal(r['semantic_preds'], b['semantic_preds'])


def test_stitch_results_numpy_thinned_masks():
    data = e2e_case(1, 30000, 2.0, 0.5, True)
    out = stitch_results(data[4], data[3], coords=data[0], gt=dict(semantic_labels=data[2]), backend='numpy')
    check_e2e(out, data, thinned=True)


def margin_only_case():
    """two tiles; tile 1 reports an instance that lies wholly in its margin (tile 0's core) and that tile 0's scan
    does not confirm"""
    xyz = np.zeros((40, 3), np.float32)
    xyz[:, 0] = np.linspace(0.05, 1.95, 40)
    tiles = tile_cloud(xyz, size=1.0, margin=0.25, origin=(0.0, 0.0), backend='numpy')
    assert len(tiles) == 2
    ids0, ids1 = tiles.point_ids
    in_margin = np.asarray(tiles.core_tile)[ids1] == 0
    assert 3 <= in_margin.sum() < ids1.size
    m0 = np.zeros(ids0.size, np.uint8)
    m0[:5] = 1
    other = np.zeros(ids1.size, np.uint8)
    other[~in_margin] = 1
    res = [dict(scan_id='s', pred_instances=[dict(scan_id='s', label_id=1, conf=0.9, pred_mask=rle_encode(m0))]),
           dict(scan_id='s', pred_instances=[dict(scan_id='s', label_id=1, conf=0.8, pred_mask=rle_encode(in_margin.astype(np.uint8))),
                                            dict(scan_id='s', label_id=1, conf=0.7, pred_mask=rle_encode(other)),
                                            dict(scan_id='s', label_id=1, conf=0.6, pred_mask=rle_encode(0 * other))])]
    return tiles, res, ids1[in_margin]


@pytest.mark.parametrize('backend', ['numpy'])
def test_drop_margin_only(backend):
    tiles, res, margin_ids = margin_only_case()
    kept = stitch_results(res, tiles, drop_margin_only=True, backend=backend)['pred_instances']
    assert [i['conf'] for i in kept] == [0.9, 0.7]
    every = stitch_results(res, tiles, drop_margin_only=False, backend=backend)['pred_instances']
    assert [i['conf'] for i in every] == [0.9, 0.8, 0.7, 0.6]
    assert np.flatnonzero(rle_decode(every[1]['pred_mask'])).tolist() == margin_ids.tolist()
    assert every[3]['pred_mask'] == dict(length=40, counts='')          # an empty mask stays


def test_stitch_results_rejects_wrong_lengths():
    data = e2e_case(*E2E_CASES[2])
    tiles, results = data[3], data[4]
    with pytest.raises(ValueError):
        stitch_results(results[:-1], tiles, backend='numpy')
    bad = list(results)
    bad[1] = dict(bad[1], semantic_preds=bad[1]['semantic_preds'][:-1])
    with pytest.raises(ValueError):
        stitch_results(bad, tiles, backend='numpy')
    bad = list(results)
    short = rle_encode(np.ones(5, np.uint8))
    bad[2] = dict(bad[2], pred_instances=[dict(scan_id='s', label_id=2, conf=0.5, pred_mask=short)])
    with pytest.raises(ValueError):
        stitch_results(bad, tiles, backend='numpy')
    with pytest.raises(ValueError):
        stitch_results(results, tiles, coords=data[0][:-1], backend='numpy')
    with pytest.raises(ValueError):
        stitch_results(results, tiles, measure='dice', backend='numpy')
