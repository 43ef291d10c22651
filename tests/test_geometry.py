"""The numpy twins of softgroup_amd.ops.geometry (the definitions the HIP kernels are held to in
tests/test_geometry_gpu.py) against independent brute forces written here: ``knn_numpy`` against a full sort of
``(d2, j)`` pairs, ``grow_segments_numpy`` against a BFS over an explicit edge set, ``point_normals_numpy`` against
analytic normals, and ``make_superpoints(backend='numpy')`` on a synthetic scene of planes and a sphere."""
import math
from collections import deque

import numpy as np
import pytest

from softgroup_amd import _lib as L
from softgroup_amd.ops import geometry as G
from softgroup_amd.util import make_superpoints

MAX_K = G.MAX_K


# ---- inputs (shared with the GPU file) -----------------------------------------------------------------------------
def random_cloud(n, seed=0, scale=1.0):
    return (np.random.default_rng(seed).random((n, 3)) * scale).astype(np.float32)


def lattice(m=6):
    """an integer lattice cast to float32: exact distance ties everywhere, at the k-th place too"""
    g = np.arange(m)
    return np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3).astype(np.float32)


def duplicates(n=200, unique=50, seed=1):
    rng = np.random.default_rng(seed)
    return random_cloud(unique, seed)[rng.integers(0, unique, n)]


SPACING = 1.0 / 16.0


def plane_scene(noise=0.0, seed=0, sphere=400):
    """a floor (z = 0), two walls (x = 0, y = 0) that meet the floor and each other at a box corner, on a dyadic grid
    of 24 x 24 points each, and a sphere above the floor -> (xyz float32 [n, 3], part int [n]: 0, 1, 2 the planes,
    3 the sphere, interior bool [n]: plane points at least three grid steps from their plane's border)"""
    g = np.arange(1, 25) * SPACING
    a, b = [v.reshape(-1) for v in np.meshgrid(g, g, indexing='ij')]
    z = np.zeros_like(a)
    t = np.arange(sphere) + 0.5
    phi, th = np.arccos(1 - 2 * t / sphere), math.pi * (1 + 5**0.5) * t
    ball = np.array([0.9, 0.9, 0.6]) + 0.4 * np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi),
                                                       np.cos(phi)], 1)
    xyz = np.concatenate([np.stack([a, b, z], 1), np.stack([z, a, b], 1), np.stack([a, z, b], 1), ball])
    part = np.concatenate([np.full(a.size, p) for p in range(3)] + [np.full(sphere, 3)])
    inner = (a >= 4 * SPACING) & (a <= 21 * SPACING) & (b >= 4 * SPACING) & (b <= 21 * SPACING)
    interior = np.concatenate([inner, inner, inner, np.zeros(sphere, bool)])
    if noise:
        xyz = xyz + np.random.default_rng(seed).normal(0.0, noise, xyz.shape)
    return xyz.astype(np.float32), part, interior


SCENE_ARGS = dict(k=16, angle=10.0, max_curvature=0.01, min_size=20)


def check_plane_segments(sp, part, interior):
    """no segment holds points of two different planes; each plane's interior lies in one segment"""
    sp = np.asarray(sp)
    for s in np.unique(sp[sp >= 0]):
        planes = np.unique(part[(sp == s) & (part < 3)])
        assert planes.size <= 1, f'segment {s} holds points of planes {planes}'
    for p in range(3):
        ids = np.unique(sp[interior & (part == p)])
        assert ids.size == 1 and ids[0] >= 0, f'the interior of plane {p} lies in segments {ids}'


# ---- brute forces ----------------------------------------------------------------------------------------------------
def knn_brute(xyz, k, max_dist=None):
    p = xyz.astype(np.float64)
    n = len(p)
    idx = np.full((n, k), -1, np.int32)
    dist = np.full((n, k), np.inf)
    for i in range(n):
        d = p[i] - p
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        order = np.lexsort((np.arange(n), d2))             # by d2, then by index
        order = order[order != i]
        if max_dist is not None:
            order = order[d2[order] <= max_dist * max_dist]
        order = order[:k]
        idx[i, :order.size] = order
        dist[i, :order.size] = d2[order]
    return idx, dist


def same_knn(got, want):
    return np.array_equal(got[0], want[0]) and got[0].dtype == np.int32 and got[1].dtype == np.float64 and \
        np.array_equal(got[1].view(np.int64), want[1].view(np.int64))


def grow_bfs(nbr, normals, curvature=None, nbr_d2=None, angle=10.0, max_curvature=None, max_dist=None, min_size=20,
             small='absorb'):
    nbr = np.asarray(nbr)
    n, k = nbr.shape
    nm = np.asarray(normals, np.float32)
    cos_thr = math.cos(math.radians(angle))
    adj = [set() for _ in range(n)]
    for i in range(n):
        for m in range(k):
            j = int(nbr[i, m])
            if j < 0 or j == i:
                continue
            if not (nm[i] != 0).any() or not (nm[j] != 0).any():
                continue
            a, b = nm[i].astype(np.float64), nm[j].astype(np.float64)
            if not abs((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) >= cos_thr:
                continue
            if max_curvature is not None and not (np.float32(curvature[i]) <= np.float32(max_curvature)
                                                  and np.float32(curvature[j]) <= np.float32(max_curvature)):
                continue
            if max_dist is not None and not nbr_d2[i, m] <= max_dist * max_dist:
                continue
            adj[i].add(j)
            adj[j].add(i)
    comp = np.full(n, -1)
    for s in range(n):                                      # ascending s: a component is met at its smallest point
        if comp[s] >= 0:
            continue
        comp[s] = s
        todo = deque([s])
        while todo:
            u = todo.popleft()
            for v in adj[u]:
                if comp[v] < 0:
                    comp[v] = s
                    todo.append(v)
    size = np.bincount(comp, minlength=n)
    number, sp = {}, np.full(n, -1, np.int32)
    for i in range(n):
        if size[comp[i]] >= min_size:
            sp[i] = number.setdefault(comp[i], len(number))
    if small == 'absorb':
        before = sp.copy()
        for i in np.flatnonzero(before < 0):
            for j in nbr[i]:
                if j >= 0 and before[j] >= 0:
                    sp[i] = before[j]
                    break
    return sp, len(number)


def flat_normals(n):
    nm = np.zeros((n, 3), np.float32)
    nm[:, 2] = 1.0
    return nm


def grow_cases():
    """name -> (nbr, normals, curvature, nbr_d2, kwargs)"""
    cases = {}
    n = 5000
    path = np.full((n, 1), -1, np.int64)
    path[:-1, 0] = np.arange(1, n)                          # i lists i + 1 only: every listing is one-directional
    cases['path'] = (path, flat_normals(n), None, None, dict(min_size=1))
    back = np.full((n, 1), -1, np.int64)
    back[1:, 0] = np.arange(n - 1)                          # the same path listed from the other end
    cases['path_back'] = (back, flat_normals(n), None, None, dict(min_size=n))
    rng = np.random.default_rng(3)
    nm = rng.normal(size=(300, 3)).astype(np.float32)       # random directions: nothing within 1 degree
    nm /= np.linalg.norm(nm, axis=1, keepdims=True)
    cases['singletons'] = (rng.integers(0, 300, (300, 4)), nm, None, None, dict(angle=1e-3, min_size=1))
    cases['singletons_dropped'] = (rng.integers(0, 300, (300, 4)), nm, None, None,
                                   dict(angle=1e-3, min_size=2, small='drop'))
    ring = np.stack([(np.arange(100) + 1) % 100, (np.arange(100) + 7) % 100], 1)
    cases['one_component'] = (ring, flat_normals(100), None, None, dict(min_size=100))
    # components of 4, 5 and 6 points (chains), min_size 5: size - 1 / size / size + 1
    chains = np.full((15, 1), -1, np.int64)
    for lo, hi in ((0, 4), (4, 9), (9, 15)):
        chains[lo:hi - 1, 0] = np.arange(lo + 1, hi)
    for small in ('drop', 'absorb'):
        cases[f'min_size_{small}'] = (chains, flat_normals(15), None, None, dict(min_size=5, small=small))
    # absorb: point 0 (alone: its normal differs) lists 1 first, which is small itself (alone too), then 2, which
    # lies in the numbered component {2 .. 7}
    nbr = np.full((8, 2), -1, np.int64)
    nbr[0] = (1, 2)
    nbr[1] = (0, -1)
    nbr[2:7, 0] = np.arange(3, 8)
    nm = flat_normals(8)
    nm[0] = (1, 0, 0)
    nm[1] = (0, 1, 0)
    cases['absorb_second'] = (nbr, nm, None, None, dict(min_size=3))
    # a point without a normal in the middle of a chain cuts it
    nm = flat_normals(9)
    nm[4] = 0
    chain = np.full((9, 1), -1, np.int64)
    chain[:-1, 0] = np.arange(1, 9)
    cases['no_normal'] = (chain, nm, None, None, dict(min_size=2, small='drop'))
    # curvature and distance limits on a random graph with smooth normals
    xyz = random_cloud(400, 5)
    idx, d2 = G.knn_numpy(xyz, 6)
    nm = flat_normals(400)
    nm[:, 0] = (0.3 * np.sin(7 * xyz[:, 0])).astype(np.float32)
    curv = rng.random(400).astype(np.float32) * 0.2
    cases['limits'] = (idx, nm, curv, d2, dict(angle=12.0, max_curvature=0.15, max_dist=0.12, min_size=4))
    cases['limits_drop'] = (idx, nm, curv, d2, dict(angle=5.0, max_curvature=0.1, min_size=3, small='drop'))
    # a clique of duplicates: every point lists every other
    dup = np.array([[j for j in range(12) if j != i] for i in range(12)])
    cases['clique'] = (dup, flat_normals(12), None, None, dict(min_size=12))
    return cases


GROW_CASES = grow_cases()


# ---- knn -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 8, MAX_K])
@pytest.mark.parametrize('cloud', ['random', 'lattice', 'duplicates'])
def test_knn_numpy_equals_full_sort(cloud, k):
    xyz = {'random': random_cloud(300, 2), 'lattice': lattice(), 'duplicates': duplicates()}[cloud]
    assert same_knn(G.knn_numpy(xyz, k), knn_brute(xyz, k))


def test_knn_numpy_lattice_has_ties_at_kth_place():
    idx, d2 = G.knn_numpy(lattice(), 4)
    inner = (d2[:, 3] == 1.0) & (np.sort(knn_brute(lattice(), 7)[1], 1)[:, 5] == 1.0)      # six at distance 1, four kept
    assert inner.any()
    assert (np.diff(idx[inner], axis=1) > 0).all()          # equal d2: ascending index


@pytest.mark.parametrize('k', [1, 5])
def test_knn_numpy_tiny_clouds(k):
    for n in (0, 1, 2, k, k + 1):
        xyz = random_cloud(n, 10 + n)
        got = G.knn_numpy(xyz, k)
        assert got[0].shape == (n, k) and same_knn(got, knn_brute(xyz, k))
        if n - 1 < k and n:
            assert (got[0][:, max(n - 1, 0):] == -1).all() and np.isinf(got[1][:, max(n - 1, 0):]).all()


@pytest.mark.parametrize('max_dist', [0.0, 0.05, 0.12, 10.0])
def test_knn_numpy_max_dist(max_dist):
    xyz = random_cloud(400, 4)
    got = G.knn_numpy(xyz, 8, max_dist=max_dist)
    assert same_knn(got, knn_brute(xyz, 8, max_dist))
    if max_dist == 0.05:
        assert (got[0] == -1).any() and (got[0][:, 0] >= 0).any()


def test_knn_numpy_ignores_cell_and_chunk():
    xyz = random_cloud(257, 6)
    want = G.knn_numpy(xyz, 8)
    assert same_knn(G.knn_numpy(xyz, 8, cell=0.01), want) and same_knn(G.knn_numpy(xyz, 8, chunk=100), want)


# ---- growth ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(GROW_CASES))
def test_grow_numpy_equals_bfs(name):
    nbr, nm, curv, d2, kw = GROW_CASES[name]
    sp, n_seg = G.grow_segments_numpy(nbr, nm, curv, d2, **kw)
    want, want_n = grow_bfs(nbr, nm, curv, d2, **kw)
    assert sp.dtype == np.int32 and np.array_equal(sp, want) and n_seg == want_n


def test_grow_cases_reach_what_they_are_for():
    out = {name: G.grow_segments_numpy(*c[:4], **c[4]) for name, c in GROW_CASES.items()}
    assert out['path'][1] == 1 and (out['path'][0] == 0).all()
    assert out['path_back'][1] == 1 and (out['path_back'][0] == 0).all()
    assert out['singletons'][1] == 300 and np.array_equal(out['singletons'][0], np.arange(300))
    assert out['singletons_dropped'][1] == 0 and (out['singletons_dropped'][0] == -1).all()
    assert out['one_component'][1] == 1
    assert out['min_size_drop'][0].tolist() == [-1] * 4 + [0] * 5 + [1] * 6
    assert out['min_size_absorb'][0].tolist() == [-1] * 4 + [0] * 5 + [1] * 6      # (the small chain lists itself only)
    assert out['absorb_second'][0].tolist() == [0, -1] + [0] * 6
    assert out['no_normal'][0].tolist() == [0] * 4 + [-1] + [1] * 4
    assert out['clique'][1] == 1
    assert 1 < out['limits'][1] and (out['limits_drop'][0] == -1).any()


def test_grow_numpy_empty():
    sp, n_seg = G.grow_segments_numpy(np.zeros((0, 3), np.int64), np.zeros((0, 3), np.float32))
    assert sp.shape == (0, ) and n_seg == 0


# ---- normals ---------------------------------------------------------------------------------------------------------
def dyadic_plane(slope):
    g = np.arange(12) / 8.0
    x, y = [v.reshape(-1) for v in np.meshgrid(g, g, indexing='ij')]
    return np.stack([x, y, slope * x], 1).astype(np.float32)


@pytest.mark.parametrize('slope,normal', [(0.0, (0.0, 0.0, 1.0)), (0.5, (-0.5 / 1.25**0.5, 0.0, 1 / 1.25**0.5))])
def test_normals_numpy_on_exact_planes(slope, normal):
    xyz = dyadic_plane(slope)
    idx, _ = G.knn_numpy(xyz, 8)
    nm, curv = G._normals_f64(xyz, idx.astype(np.int64), 3)
    assert np.abs(nm - np.array(normal)).max() <= 1e-12 and np.abs(curv).max() <= 1e-12
    nm32, curv32 = G.point_normals_numpy(xyz, idx)
    assert nm32.dtype == np.float32 and curv32.dtype == np.float32 and nm32.shape == (len(xyz), 3)
    assert np.array_equal(nm32, nm.astype(np.float32))


def test_normals_numpy_too_few_neighbours_and_coincident_support():
    xyz = dyadic_plane(0.0)
    idx, _ = G.knn_numpy(xyz, 8)
    idx[5, 2:] = -1                                         # two valid neighbours < 3
    idx[6, 3:] = -1                                         # three: just enough
    nm, curv = G.point_normals_numpy(xyz, idx, min_neighbours=3)
    assert (nm[5] == 0).all() and curv[5] == 0 and (nm[6] != 0).any()
    same = np.zeros((4, 3), np.float32) + np.float32(0.3)   # all points coincide: the eigenvalue sum is 0
    nm, curv = G.point_normals_numpy(same, G.knn_numpy(same, 3)[0])
    assert (nm == 0).all() and (curv == 0).all()


def test_normals_numpy_sign_rule():
    rng = np.random.default_rng(8)
    xyz = rng.normal(size=(300, 3)).astype(np.float32)
    nm, curv = G.point_normals_numpy(xyz, G.knn_numpy(xyz, 8)[0])
    lead = np.abs(nm).argmax(1)
    assert (nm[np.arange(300), lead] > 0).all()
    assert np.abs(np.linalg.norm(nm.astype(np.float64), axis=1) - 1).max() < 1e-6
    assert (curv >= 0).all() and (curv <= 1 / 3 + 1e-6).all()
    # the mirrored cloud lies in the same plane: the same normal, z (its greatest component) positive
    tilted = dyadic_plane(0.5) * np.float32(-1)
    nm, _ = G.point_normals_numpy(tilted, G.knn_numpy(tilted, 8)[0])
    assert (nm[:, 2] > 0).all()


# ---- make_superpoints ------------------------------------------------------------------------------------------------
def test_make_superpoints_numpy_on_plane_scene():
    xyz, part, interior = plane_scene()
    sp = make_superpoints(xyz, backend='numpy', small='drop', **SCENE_ARGS)
    assert sp.dtype == np.int32 and sp.shape == (len(xyz), )
    check_plane_segments(sp, part, interior)
    sp2, nm, curv, idx = make_superpoints(xyz, backend='numpy', small='drop', return_geometry=True, **SCENE_ARGS)
    assert np.array_equal(sp, sp2) and nm.shape == (len(xyz), 3) and curv.shape == (len(xyz), )
    assert idx.shape == (len(xyz), SCENE_ARGS['k'])
    floor = interior & (part == 0)
    assert np.array_equal(nm[floor], np.tile(np.float32([0, 0, 1]), (floor.sum(), 1)))
    # what comes out goes into the index of the snap stage as it is
    from softgroup_amd.ops import superpoint_index_numpy
    index = superpoint_index_numpy(make_superpoints(xyz, backend='numpy', **SCENE_ARGS))
    assert index.n_seg >= 3 and index.n_points == len(xyz)


# ---- the C ABI and argument errors -------------------------------------------------------------------------------------
def test_ctypes_table_covers_the_geometry_symbols():
    names = ['sg_knn_default_cell', 'sg_knn_workspace_bytes', 'sg_knn', 'sg_point_normals',
             'sg_grow_segments_workspace_bytes', 'sg_grow_segments']
    lib = L.lib()
    for name in names:
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert lib.sg_knn_workspace_bytes(1000, MAX_K) > 0
    assert lib.sg_knn_workspace_bytes(1000, MAX_K + 1) == 0 and lib.sg_knn_workspace_bytes(1000, 0) == 0
    assert lib.sg_knn_workspace_bytes(2**31, 8) == 0 and lib.sg_grow_segments_workspace_bytes(2**31) == 0
    # out of range: a negative status and a message, nothing launched (no GPU is needed to get here)
    assert lib.sg_knn(None, 10, MAX_K + 1, 1.0, -1.0, None, None, None, None, 0, None) < 0
    assert b'sg_knn' in lib.sg_last_error()
    assert lib.sg_knn(None, 2**31, 8, 1.0, -1.0, None, None, None, None, 0, None) < 0
    assert lib.sg_point_normals(None, 2**31, None, 8, 3, None, None, None, None) < 0
    assert lib.sg_grow_segments(None, None, 10, 0, None, None, 0.9, 0.0, -1.0, 20, 1, None, None, None, 0, None) < 0
    assert b'sg_grow_segments' in lib.sg_last_error()


def test_default_cell_heuristic():
    lo, hi = np.zeros(3), np.array([2.0, 2.0, 2.0])
    assert G.knn_default_cell(lo, hi, 8000, 16) == pytest.approx((8 * 8.0 / 8000) ** (1 / 3))
    assert G.knn_default_cell(lo, np.array([2.0, 2.0, 0.0]), 400, 8) == pytest.approx((4 * 4.0 / 400) ** 0.5)
    assert G.knn_default_cell(lo, lo, 5, 8) == 1.0
    assert G.knn_default_cell(lo, np.array([2.0**40, 1.0, 1.0]), 10**6, 8) >= 2.0**11


def test_argument_errors():
    xyz = random_cloud(20)
    idx, d2 = G.knn_numpy(xyz, 4)
    nm = flat_normals(20)
    bad = xyz.copy()
    bad[3, 1] = np.nan
    far = xyz.copy()
    far[0, 0] = 1e9
    for call in (lambda: G.knn_numpy(xyz, 0), lambda: G.knn_numpy(xyz, MAX_K + 1), lambda: G.knn(xyz, 2.5),
                 lambda: G.knn(xyz, 4, backend='cuda'), lambda: G.knn_numpy(xyz[:, :2], 4),
                 lambda: G.knn_numpy(bad, 4), lambda: G.knn(bad, 4, backend='numpy'),
                 lambda: G.knn_numpy(far, 4, cell=0.5), lambda: G.knn_numpy(xyz, 4, cell=0.0),
                 lambda: G.knn_numpy(xyz, 4, max_dist=-1.0),
                 lambda: G.point_normals_numpy(xyz, idx[:10]), lambda: G.point_normals_numpy(xyz, idx + 17),
                 lambda: G.point_normals_numpy(xyz, idx - 2), lambda: G.point_normals_numpy(xyz, idx, min_neighbours=-1),
                 lambda: G.grow_segments_numpy(idx, nm, angle=100.0), lambda: G.grow_segments_numpy(idx, nm, small='keep'),
                 lambda: G.grow_segments_numpy(idx, nm, min_size=0), lambda: G.grow_segments_numpy(idx, nm, max_dist=0.1),
                 lambda: G.grow_segments_numpy(idx, nm, max_curvature=0.1),
                 lambda: G.grow_segments_numpy(idx + 17, nm), lambda: G.grow_segments_numpy(idx, nm[:, :2]),
                 lambda: make_superpoints(xyz, k=0, backend='numpy'),
                 lambda: make_superpoints(bad, backend='numpy')):
        with pytest.raises(ValueError):
            call()
