"""``sg_knn``, ``sg_point_normals`` and ``sg_grow_segments`` on the device: through ctypes into poisoned buffers with
spare rows behind them and a dirty workspace, and through the Python surface, against the numpy twins that
tests/test_geometry.py checks against brute forces.  knn and the growth: equality of every byte, and of two runs.
The normals: the bound the eigen-solvers allow (see ``test_normals_against_twin``).

Launch grids: no kernel of geometry.hip caps its grid except the full scan of the work list (2048 workgroups stride
over it); ``test_knn_cell_extremes`` lists 3000 queries, so that loop runs more than once."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from softgroup_amd import _lib as L
from softgroup_amd import ops, synthetic
from softgroup_amd.ops import geometry as G
from softgroup_amd.util import make_superpoints, refine_result

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_geometry import (GROW_CASES, SCENE_ARGS, check_plane_segments, duplicates, lattice,  # noqa: E402
                           plane_scene, random_cloud, same_knn)
from test_mask_split import instance_list  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
POISON_D2 = -7.25
SPARE = 3
MAX_K = G.MAX_K
DEV = torch.device('cuda')


def dirty_ws(nbytes):
    assert nbytes > 0
    return torch.full((nbytes, ), 0x5A, dtype=torch.uint8, device=DEV)


def up(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def default_cell(xyz, k):
    return G.knn_default_cell(xyz.min(0), xyz.max(0), len(xyz), k) if len(xyz) else 1.0


# ---- knn through ctypes ------------------------------------------------------------------------------------------------
def run_knn(xyz, k, cell, max_dist=None):
    """-> (rc, meta, idx [N, k], d2 [N, k], untouched): SPARE rows behind the outputs, checked"""
    lib = L.lib()
    N = len(xyz)
    d_xyz = up(xyz, np.float32)
    idx = torch.full((N + SPARE, k), POISON, dtype=torch.int32, device=DEV)
    d2 = torch.full((N + SPARE, k), POISON_D2, dtype=torch.float64, device=DEV)
    meta = torch.full((4, ), -77, dtype=torch.int32, device=DEV)
    nb = lib.sg_knn_workspace_bytes(N, k)
    ws = dirty_ws(nb)
    rc = lib.sg_knn(L.ptr(d_xyz) if N else None, N, k, float(cell), -1.0 if max_dist is None else float(max_dist),
                    L.ptr(idx), L.ptr(d2), L.ptr(meta), L.ptr(ws), nb, L.stream())
    torch.cuda.synchronize()
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    assert (idx[N:] == POISON).all() and (d2[N:] == POISON_D2).all(), 'written behind the outputs'
    return rc, meta.cpu().tolist(), idx[:N], d2[:N]


def check_knn(xyz, k, cell, max_dist=None, want=None):
    """the device equals the twin byte for byte, twice -> meta"""
    want = want if want is not None else G.knn_numpy(xyz, k, max_dist=max_dist)
    rc, meta, idx, d2 = run_knn(xyz, k, cell, max_dist)
    assert rc == 0 and meta[1:] == [0, 0, 0] and 0 <= meta[0] <= len(xyz)
    assert same_knn((idx, d2), want)
    rc2, meta2, idx2, d22 = run_knn(xyz, k, cell, max_dist)
    assert rc2 == 0 and meta2 == meta and same_knn((idx2, d22), (idx, d2))
    return meta


_REFERENCE = {}


def reference(n):
    """cloud and its MAX_K neighbours, computed once; the first k columns are the k neighbours"""
    if n not in _REFERENCE:
        xyz = random_cloud(n, 40 + n % 7)
        _REFERENCE[n] = (xyz, G.knn_numpy(xyz, MAX_K))
    return _REFERENCE[n]


@pytest.mark.parametrize('k', [1, 8, MAX_K])
@pytest.mark.parametrize('n', [0, 1, 2, 33, 3000, 20000])
def test_knn_equals_twin(n, k):
    xyz, (idx, d2) = reference(n)
    want = (np.ascontiguousarray(idx[:, :k]), np.ascontiguousarray(d2[:, :k]))
    if n - 1 < MAX_K:                                         # (a short row is not a prefix of a long one's layout)
        want = G.knn_numpy(xyz, k)
    check_knn(xyz, k, default_cell(xyz, k), want=want)


@pytest.mark.parametrize('k', [8, MAX_K])
@pytest.mark.parametrize('cloud', ['lattice', 'duplicates', 'faces'])
def test_knn_ties_and_cell_faces(cloud, k):
    if cloud == 'faces':      # every coordinate a multiple of the cell, a power of two: points exactly on cell faces
        xyz = (np.random.default_rng(9).integers(-8, 8, (600, 3)) * 0.25).astype(np.float32)
        cells = [0.25]
    else:
        xyz = lattice() if cloud == 'lattice' else duplicates()
        cells = [1.0, default_cell(xyz, k)]
    want = G.knn_numpy(xyz, k)
    for cell in cells:
        check_knn(xyz, k, cell, want=want)


def test_knn_cell_extremes():
    xyz, (idx, d2) = reference(3000)
    want = (np.ascontiguousarray(idx[:, :8]), np.ascontiguousarray(d2[:, :8]))
    meta = check_knn(xyz, 8, 1e-4, want=want)                 # every point alone in its cell, nothing within 3 shells
    assert meta[0] == 3000                                    # all of them scanned: more queries than scan workgroups
    meta = check_knn(xyz, 8, 64.0, want=want)                 # all points in one cell
    assert meta[0] == 0


@pytest.mark.parametrize('k', [8, MAX_K])
def test_knn_clusters_and_isolated_point_reach_the_full_scan(k):
    rng = np.random.default_rng(12)
    cell = 0.02
    a = rng.random((500, 3)) * 0.05
    b = rng.random((500, 3)) * 0.05 + np.array([1000 * cell, 0, 0])
    xyz = np.concatenate([a, b, [[500 * cell, 300 * cell, -200 * cell]]]).astype(np.float32)
    meta = check_knn(xyz, k, cell)
    assert 1 <= meta[0] < len(xyz), 'the isolated point is scanned, the clusters are not'


@pytest.mark.parametrize('max_dist,cell', [(0.04, 0.05), (0.04, 0.01), (0.5, 0.05), (0.0, 0.05)])
def test_knn_max_dist(max_dist, cell):
    """the 8th neighbour of this cloud lies at about 0.086: 0.04 cuts rows short, 0.5 does not; cell 0.05 bounds the
    walk by max_dist (no scan), cell 0.01 does not (4 shells > the cap: the scan answers with the limit)"""
    xyz, _ = reference(3000)
    meta = check_knn(xyz, 8, cell, max_dist=max_dist)
    if max_dist <= 0.04 and cell == 0.05:
        assert meta[0] == 0
    if cell == 0.01:
        assert meta[0] > 0


@pytest.mark.parametrize('bad,flag', [(np.nan, 1), (np.inf, 1), (3e9, 4)])
def test_knn_invalid_coordinate_touches_no_row(bad, flag):
    xyz = random_cloud(500, 3)
    xyz[321, 1] = bad
    rc, meta, idx, d2 = run_knn(xyz, 8, 0.5)
    assert rc == 0 and meta == [0, flag, 0, 0]
    assert (idx == POISON).all() and (d2 == POISON_D2).all()
    for cell in (0.5, None) if flag == 1 else (0.5, ):
        with pytest.raises(ValueError):
            ops.knn(torch.from_numpy(xyz).to(DEV), 8, cell=cell)


def test_knn_python_surface():
    xyz, (idx, d2) = reference(3000)
    want = (np.ascontiguousarray(idx[:, :16]), np.ascontiguousarray(d2[:, :16]))
    got = ops.knn(torch.from_numpy(xyz).to(DEV), 16)
    assert got[0].is_cuda and got[0].dtype == torch.int32 and got[1].dtype == torch.float64
    assert same_knn((got[0].cpu().numpy(), got[1].cpu().numpy()), want)
    got = ops.knn(xyz, 16, backend='device', cell=0.1, return_meta=True)
    assert isinstance(got[0], np.ndarray) and same_knn(got[:2], want) and got[2] >= 0
    empty = ops.knn(torch.zeros((0, 3), device=DEV), 4)
    assert tuple(empty[0].shape) == (0, 4) and tuple(empty[1].shape) == (0, 4)
    with pytest.raises(ValueError):
        ops.knn(torch.from_numpy(xyz).to(DEV), MAX_K + 1)


# ---- the growth through ctypes ---------------------------------------------------------------------------------------
def run_grow(nbr, normals, curvature=None, nbr_d2=None, angle=10.0, max_curvature=None, max_dist=None, min_size=20,
             small='absorb'):
    """-> (meta, sp [N])"""
    lib = L.lib()
    N, k = nbr.shape
    d_nbr, d_nm = up(nbr, np.int32), up(normals, np.float32)
    d_curv = up(curvature, np.float32) if max_curvature is not None else None
    d_d2 = up(nbr_d2, np.float64) if max_dist is not None else None
    sp = torch.full((N + SPARE, ), POISON, dtype=torch.int32, device=DEV)
    meta = torch.full((4, ), -77, dtype=torch.int32, device=DEV)
    nb = lib.sg_grow_segments_workspace_bytes(N)
    ws = dirty_ws(nb)
    L.check(lib.sg_grow_segments(L.ptr(d_nbr), L.ptr(d_d2), N, k, L.ptr(d_nm), L.ptr(d_curv),
                                 math.cos(math.radians(angle)), 0.0 if max_curvature is None else float(max_curvature),
                                 -1.0 if max_dist is None else float(max_dist), min_size, int(small == 'absorb'),
                                 L.ptr(sp), L.ptr(meta), L.ptr(ws), nb, L.stream()), 'sg_grow_segments')
    torch.cuda.synchronize()
    sp = sp.cpu().numpy()
    assert (sp[N:] == POISON).all(), 'written behind the output'
    return meta.cpu().tolist(), sp[:N]


def check_grow(nbr, normals, curvature, nbr_d2, kw):
    want, n_seg = G.grow_segments_numpy(nbr, normals, curvature, nbr_d2, **kw)
    components = G.grow_segments_numpy(nbr, normals, curvature, nbr_d2, **dict(kw, min_size=1, small='drop'))[1]
    meta, sp = run_grow(nbr, normals, curvature, nbr_d2, **kw)
    assert meta == [n_seg, 0, components, 0]
    assert np.array_equal(sp, want)
    meta2, sp2 = run_grow(nbr, normals, curvature, nbr_d2, **kw)
    assert meta2 == meta and np.array_equal(sp2, sp)
    return n_seg


@pytest.mark.parametrize('name', sorted(GROW_CASES))
def test_grow_equals_twin(name):
    nbr, nm, curv, d2, kw = GROW_CASES[name]
    check_grow(nbr, nm, curv, d2, kw)


@pytest.fixture(scope='module')
def room():
    """a 20 000-point room with the device's neighbours (held to the twin above) and the TWIN's normals"""
    xyz = synthetic.scene_s2(seed=3, n=20000, room_scale=0.37)[0].astype(np.float32)
    idx, d2 = ops.knn(xyz, 16, backend='device')
    nm, curv = G.point_normals_numpy(xyz, idx)
    return xyz, idx, d2, nm, curv


@pytest.mark.parametrize('kw', [dict(), dict(max_curvature=0.02, small='drop'), dict(angle=4.0, max_dist=0.03, min_size=50)])
def test_grow_room_equals_twin(room, kw):
    xyz, idx, d2, nm, curv = room
    assert check_grow(idx, nm, curv, d2, kw) >= 2


def test_grow_python_surface_and_bad_index(room):
    xyz, idx, d2, nm, curv = room
    want, n_seg = G.grow_segments_numpy(idx, nm, curv, d2, max_curvature=0.05, max_dist=0.05)
    sp, n = ops.grow_segments(up(idx, np.int32), up(nm, np.float32), up(curv, np.float32), up(d2, np.float64),
                              max_curvature=0.05, max_dist=0.05)
    assert sp.is_cuda and sp.dtype == torch.int32 and n == n_seg and np.array_equal(sp.cpu().numpy(), want)
    sp, n = ops.grow_segments(idx, nm, curv, d2, max_curvature=0.05, max_dist=0.05, backend='device')
    assert isinstance(sp, np.ndarray) and n == n_seg and np.array_equal(sp, want)
    # an index outside -1 .. N - 1 is never dereferenced: it counts as -1 and sets the flag
    N = len(idx)
    bad = idx.copy()
    hit = np.flatnonzero(bad[:, 0] >= 0)[:3]
    bad[hit[0], 0], bad[hit[1], 0], bad[hit[2], 0] = N, 2**31 - 1, -5
    clean = bad.copy()
    clean[hit, 0] = -1
    meta, got = run_grow(bad, nm)
    assert meta[1] == 1 and np.array_equal(got, G.grow_segments_numpy(clean, nm)[0])
    with pytest.raises(ValueError):
        ops.grow_segments(up(bad, np.int32), up(nm, np.float32))
    with pytest.raises(ValueError):
        ops.point_normals(up(xyz, np.float32), up(bad, np.int32))
    sp, n = ops.grow_segments(torch.zeros((0, 4), dtype=torch.int32, device=DEV), torch.zeros((0, 3), device=DEV))
    assert sp.numel() == 0 and n == 0


# ---- normals -----------------------------------------------------------------------------------------------------------
def run_normals(xyz, nbr, min_neighbours=3):
    lib = L.lib()
    N, k = nbr.shape
    d_xyz, d_nbr = up(xyz, np.float32), up(nbr, np.int32)
    nm = torch.full((N + SPARE, 3), -7.25, dtype=torch.float32, device=DEV)
    curv = torch.full((N + SPARE, ), -7.25, dtype=torch.float32, device=DEV)
    meta = torch.full((4, ), -77, dtype=torch.int32, device=DEV)
    L.check(lib.sg_point_normals(L.ptr(d_xyz), N, L.ptr(d_nbr), k, min_neighbours, L.ptr(nm), L.ptr(curv), L.ptr(meta),
                                 L.stream()), 'sg_point_normals')
    torch.cuda.synchronize()
    nm, curv = nm.cpu().numpy(), curv.cpu().numpy()
    assert (nm[N:] == -7.25).all() and (curv[N:] == -7.25).all(), 'written behind the outputs'
    return meta.cpu().tolist(), nm[:N], curv[:N]


@pytest.mark.parametrize('k', [8, 16])
def test_normals_against_twin(k):
    """Bound: the float32 rounding of a unit vector moves it by at most about 1.1e-7 rad, a double eigen-solve at a
    relative gap of 1e-3 adds about 2^-52 / 1e-3: 1e-6 rad leaves a tenfold margin.  The angle is asin(|n x m|), which
    keeps its digits near 0 (arccos of the dot product does not)."""
    xyz, part, interior = plane_scene(noise=0.003, seed=k)
    idx, _ = G.knn_numpy(xyz, k)
    idx = idx.copy()
    idx[::97, 2:] = -1                                         # a few points below min_neighbours
    want_nm, want_curv = G.point_normals_numpy(xyz, idx)
    _, _, lam = G._normals_f64(xyz, idx.astype(np.int64), 3, return_eigenvalues=True)
    meta, nm, curv = run_normals(xyz, idx)
    none = (want_nm == 0).all(1)
    assert none.sum() == len(range(0, len(xyz), 97)) and meta == [int(none.sum()), 0, 0, 0]
    assert np.array_equal((nm == 0).all(1), none) and (curv[none] == 0).all()
    with np.errstate(invalid='ignore', divide='ignore'):
        gap = (lam[:, 1] - lam[:, 0]) / lam[:, 2]
    judged = ~none & (gap >= 1e-3)
    excluded = (~none & ~judged).sum() / len(xyz)
    a, b = nm.astype(np.float64), want_nm.astype(np.float64)
    angle = np.arcsin(np.minimum(np.linalg.norm(np.cross(a, b), axis=1), 1.0))
    diff = np.abs(curv.astype(np.float64) - want_curv.astype(np.float64))
    print(f'k {k}: worst angle {angle[judged].max():.3e} rad, worst curvature difference {diff.max():.3e}, '
          f'excluded {100 * excluded:.2f} %')
    assert excluded <= 0.01
    assert angle[judged].max() <= 1e-6
    assert diff.max() <= 1e-6
    lead = np.abs(nm[~none]).argmax(1)
    assert (nm[~none][np.arange(lead.size), lead] > 0).all()  # the sign rule
    meta2, nm2, curv2 = run_normals(xyz, idx)
    assert meta2 == meta and np.array_equal(nm2, nm) and np.array_equal(curv2, curv)


def test_normals_python_surface():
    xyz, _, _ = plane_scene()
    idx, _ = G.knn_numpy(xyz, 8)
    nm, curv = ops.point_normals(up(xyz, np.float32), up(idx, np.int32))
    assert nm.is_cuda and nm.dtype == torch.float32 and tuple(nm.shape) == (len(xyz), 3) and curv.dtype == torch.float32
    nm2, curv2 = ops.point_normals(xyz, idx, backend='device')
    assert isinstance(nm2, np.ndarray) and np.array_equal(nm2, nm.cpu().numpy()) and np.array_equal(curv2, curv.cpu().numpy())
    floor = np.flatnonzero((xyz[:, 2] == 0) & (xyz[:, 0] >= 0.25) & (xyz[:, 1] >= 0.25) & (xyz[:, 0] <= 1.25) & (xyz[:, 1] <= 1.25))
    assert np.array_equal(nm2[floor], np.tile(np.float32([0, 0, 1]), (floor.size, 1))) and (curv2[floor] == 0).all()
    nm0, curv0 = ops.point_normals(torch.zeros((0, 3), device=DEV), torch.zeros((0, 8), dtype=torch.int32, device=DEV))
    assert nm0.numel() == 0 and curv0.numel() == 0


# ---- make_superpoints ----------------------------------------------------------------------------------------------------
def test_make_superpoints_device_on_plane_scene():
    xyz, part, interior = plane_scene()
    d_xyz = torch.from_numpy(xyz).to(DEV)
    for small in ('drop', 'absorb'):
        # noise-free and dyadic: every link decision is far from its threshold, the two backends agree exactly
        want = make_superpoints(xyz, backend='numpy', small=small, **SCENE_ARGS)
        sp = make_superpoints(d_xyz, small=small, **SCENE_ARGS)
        assert sp.is_cuda and sp.dtype == torch.int32
        assert np.array_equal(sp.cpu().numpy(), want)
        assert np.array_equal(make_superpoints(xyz, backend='device', small=small, **SCENE_ARGS), want)
    check_plane_segments(make_superpoints(d_xyz, small='drop', **SCENE_ARGS).cpu().numpy(), part, interior)
    sp, nm, curv, idx = make_superpoints(d_xyz, return_geometry=True, **SCENE_ARGS)
    assert nm.is_cuda and curv.is_cuda and idx.is_cuda and tuple(idx.shape) == (len(xyz), SCENE_ARGS['k'])


def test_make_superpoints_noisy_scene_feeds_the_snap_stage():
    xyz, part, interior = plane_scene(noise=0.003, seed=2)
    d_xyz = torch.from_numpy(xyz).to(DEV)
    sp = make_superpoints(d_xyz, small='drop', **SCENE_ARGS)
    check_plane_segments(sp.cpu().numpy(), part, interior)
    sp = make_superpoints(d_xyz, **SCENE_ARGS)
    index = ops.superpoint_index(sp)
    assert index.is_cuda and index.n_points == len(xyz) and index.n_seg >= 3
    # masks = the planes with a few points knocked out and stray points added; labels = the part with salt noise
    rng = np.random.default_rng(4)
    dense = np.stack([part == p for p in range(4)])
    dense ^= rng.random(dense.shape) < 0.03
    sem = np.where(rng.random(len(xyz)) < 0.05, rng.integers(0, 4, len(xyz)), part).astype(np.int64)
    result = dict(scan_id='s', semantic_preds=sem, pred_instances=instance_list(dense))
    got = refine_result(result, sp, n_classes=4, backend='device')
    want = refine_result(result, sp.cpu().numpy(), n_classes=4, backend='numpy')
    assert np.array_equal(got['semantic_preds'], want['semantic_preds'])
    assert [g['pred_mask'] for g in got['pred_instances']] == [w['pred_mask'] for w in want['pred_instances']]
    clean = (got['semantic_preds'] == part)[interior].mean()
    assert clean > (sem == part)[interior].mean()             # the vote repaired labels inside the planes
