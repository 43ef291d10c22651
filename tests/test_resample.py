"""Voxel / random downsample, exact nearest source point, masks through an index map and ``propagate_result``:
the numpy paths against independent brute-force restatements written HERE -- a Python dict keyed by the cell tuple
that keeps the best (d2, i) for the voxels, a chunked float64 distance matrix with ``argmin`` for the nearest point,
dense bool arrays for the masks.  Equality everywhere, no tolerances.  tests/test_resample_gpu.py holds the HIP
kernels to the same references on the same inputs.  (None of these modules exists before this feature.)"""
import functools
import importlib.util
import os
import random

import numpy as np
import pytest
import torch

from softgroup_amd.data import apply_sample, random_downsample, voxel_downsample
from softgroup_amd.ops import resample as RS
from softgroup_amd.util import propagate_result, rle_decode, rle_encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 70001
VOXELS = [0.25, 0.02, 0.05, 1.0]       # exactly representable (points ON cell faces); not representable (x2); many waves per voxel
MIN_TIES = {0.25: 50, 0.02: 20, 0.05: 20}
PICKS = ['first', 'center']
EDGE_N = [0, 1, 257]
CELLS = [None, 1e-3, 0.05, 10.0]
N_QUERY = 8192


@functools.lru_cache(maxsize=None)
def cloud():
    """uniform in an 8 x 6 x 3 m box centred on the origin, snapped to a 1/64 m lattice: ties are real"""
    rng = np.random.default_rng(7)
    x = (rng.random((N, 3)) - 0.5) * np.array([8.0, 6.0, 3.0])
    x = (np.round(x * 64) / 64).astype(np.float32)
    x.setflags(write=False)
    return x


# ---- voxels -----------------------------------------------------------------------------------------------------------
def brute_voxels(xyz, voxel, pick):
    """-> (sample_ids, inverse, n_tie_voxels): a dict keyed by the cell tuple, a loop that keeps the best (d2, i)"""
    x = xyz.astype(np.float64)
    c = np.floor(x / voxel)
    d = x - (c + 0.5) * voxel
    d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).tolist()
    keys = [tuple(r) for r in c.astype(np.int64).tolist()]
    best, ties = {}, {}
    for i, k in enumerate(keys):
        v = 0.0 if pick == 'first' else d2[i]
        b = best.get(k)
        if b is None or v < b[0]:           # (ascending i: an equal value never replaces the lower index)
            best[k] = (v, i)
            ties[k] = 1
        elif v == b[0]:
            ties[k] += 1
    ids = np.array(sorted(b[1] for b in best.values()), dtype=np.int64)
    pos = {int(i): p for p, i in enumerate(ids.tolist())}
    inverse = np.array([pos[best[k][1]] for k in keys], dtype=np.int64)
    return ids, inverse, sum(1 for t in ties.values() if t >= 2)


@functools.lru_cache(maxsize=None)
def voxel_reference(voxel, pick):
    return brute_voxels(cloud(), voxel, pick)


def edge_cloud(n):
    if n == 64:
        return np.tile(np.array([[0.375, -1.25, 2.0]], np.float32), (64, 1))      # 64 identical points
    return cloud()[5000:5000 + n].copy()


def check_voxels(ids, inverse, ref):
    """ascending, consistent, equal to the brute force"""
    want_ids, want_inverse, _ = ref
    ids, inverse = np.asarray(ids), np.asarray(inverse)
    assert ids.dtype == np.int64 and inverse.dtype == np.int64
    assert (np.diff(ids) > 0).all()
    assert inverse.size == 0 or (0 <= inverse.min() and inverse.max() < ids.size)
    assert np.array_equal(np.unique(inverse), np.arange(ids.size))
    assert np.array_equal(inverse[ids], np.arange(ids.size))
    assert np.array_equal(ids, want_ids) and np.array_equal(inverse, want_inverse)


BAD_CLOUDS = {      # (row 1 is the invalid point)
    'nan': (np.array([[0, 0, 0], [1, np.nan, 0], [2, 2, 2]], np.float32), 0.25),
    'inf': (np.array([[0, 0, 0], [-np.inf, 2, 2], [1, 1, 1]], np.float32), 0.25),
    'range': (np.array([[0, 0, 0], [1e12, 1, 1], [2, 2, 2]], np.float32), 1e-3),
}


@pytest.mark.parametrize('voxel', VOXELS)
def test_cloud_has_the_ties_the_rules_are_about(voxel):
    ids, _, tie_voxels = voxel_reference(voxel, 'center')
    if voxel in MIN_TIES:
        assert tie_voxels >= MIN_TIES[voxel]
    if voxel == 1.0:
        assert ids.size * 256 <= N              # hundreds of points per voxel on average: a voxel spans many waves
    if voxel == 0.25:                          # points exactly on cell faces
        assert (np.mod(cloud().astype(np.float64), 0.25) == 0).any(1).sum() > 1000


@pytest.mark.parametrize('pick', PICKS)
@pytest.mark.parametrize('voxel', VOXELS)
def test_voxel_downsample_numpy_equals_brute_force(voxel, pick):
    ids, inverse = voxel_downsample(cloud(), voxel, pick=pick, backend='numpy')
    check_voxels(ids, inverse, voxel_reference(voxel, pick))


@pytest.mark.parametrize('pick', PICKS)
@pytest.mark.parametrize('n', EDGE_N + [64])
def test_voxel_downsample_numpy_edge_sizes(n, pick):
    x = edge_cloud(n)
    ids, inverse = voxel_downsample(x, 0.25, pick=pick, backend='numpy')
    check_voxels(ids, inverse, brute_voxels(x, 0.25, pick))
    if n == 64:
        assert ids.tolist() == [0] and not inverse.any()


@pytest.mark.parametrize('name', sorted(BAD_CLOUDS))
def test_voxel_downsample_numpy_rejects_invalid_points(name):
    x, voxel = BAD_CLOUDS[name]
    with pytest.raises(ValueError):
        voxel_downsample(x, voxel, backend='numpy')
    with pytest.raises(ValueError):
        voxel_downsample(cloud()[:10], 0.0, backend='numpy')
    with pytest.raises(ValueError):
        voxel_downsample(cloud()[:10], 0.1, pick='mean', backend='numpy')


def test_voxel_downsample_keeps_the_input_kind():
    ids, inverse = voxel_downsample(torch.from_numpy(cloud()[:300].copy()), 0.5, backend='numpy')
    assert torch.is_tensor(ids) and ids.dtype == torch.int64 and inverse.dtype == torch.int64
    check_voxels(ids.numpy(), inverse.numpy(), brute_voxels(cloud()[:300], 0.5, 'center'))


def test_random_downsample_is_the_reference_draw():
    ids = random_downsample(1000, 0.25, seed=3)
    assert ids.dtype == np.int64 and ids.tolist() == random.Random(3).sample(range(1000), 250)
    assert random_downsample(7, 0.5, seed=0).size == 3          # int(n * ratio)
    assert random_downsample(0, 0.5, seed=0).size == 0
    with pytest.raises(ValueError):
        random_downsample(10, 0.5, rng='numpy')
    xyz, rgb = cloud()[:1000], np.arange(3000, dtype=np.uint8).reshape(1000, 3)
    sem, ins = np.arange(1000), -np.arange(1000)
    a, b, c, d = apply_sample(ids, xyz, rgb, sem, ins)
    assert np.array_equal(a, xyz[ids]) and np.array_equal(b, rgb[ids]) and b.dtype == np.uint8
    assert np.array_equal(c, ids) and np.array_equal(d, -ids)


# ---- nearest point ---------------------------------------------------------------------------------------------------
def brute_nearest(src, query, max_dist=None, chunk=512):
    """-> (index, d2, ties per query): float64 distance matrix in chunks, argmin (the first, lowest, index)"""
    s = src.astype(np.float64)
    index = np.empty(len(query), np.int64)
    d2_min = np.empty(len(query), np.float64)
    ties = np.empty(len(query), np.int64)
    for lo in range(0, len(query), chunk):
        q = query[lo:lo + chunk].astype(np.float64)
        dx, dy, dz = (q[:, None, k] - s[None, :, k] for k in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        index[lo:lo + chunk] = d2.argmin(1)
        d2_min[lo:lo + chunk] = d2.min(1)
        ties[lo:lo + chunk] = (d2 == d2.min(1, keepdims=True)).sum(1)
    if max_dist is not None:
        far = d2_min > max_dist * max_dist
        index[far] = -1
        d2_min[far] = np.inf
    return index, d2_min, ties


@functools.lru_cache(maxsize=None)
def nearest_inputs():
    """sources: the sorted reference draw of a quarter of the cloud; queries: its first 8192 points"""
    ids = np.array(sorted(random.Random(0).sample(range(N), N // 4)), dtype=np.int64)
    return ids, cloud()[ids], cloud()[:N_QUERY]


@functools.lru_cache(maxsize=None)
def nearest_reference():
    _, src, query = nearest_inputs()
    return brute_nearest(src, query)


@functools.lru_cache(maxsize=None)
def nearest_cases():
    """name -> (src, query, max_dist): the small cases, each with its own brute force"""
    rng = np.random.default_rng(11)
    a = rng.normal(0, 0.3, (300, 3))
    b = rng.normal(0, 0.3, (300, 3)) + np.array([500.0, 0, 0])
    clusters = np.concatenate([a, b]).astype(np.float32)
    between = np.concatenate([rng.uniform(-5, 505, (256, 1)), rng.normal(0, 3, (256, 2))], 1)
    around = np.concatenate([a[:128] + rng.normal(0, 0.05, (128, 3)), b[:128] + rng.normal(0, 0.05, (128, 3))])
    _, src, query = nearest_inputs()
    far = query[:256].copy()
    far[:64] += np.float32(1000.0)
    dup = np.concatenate([src[:500], src[:500][::-1], src[:500]])          # every source three times
    return {
        'two_clusters': (clusters, np.concatenate([between, around]).astype(np.float32), None),
        'far_queries': (src[:4000], far, None),
        'one_source': (src[7:8], query[:300], None),
        'no_query': (src[:100], np.zeros((0, 3), np.float32), None),
        'duplicate_sources': (dup, np.concatenate([src[:400], query[:200]]), None),
        'max_dist_small': (src[:2000], query[:500], 0.05),
    }


def test_nearest_inputs_have_ties_and_exact_hits():
    ids, _, _ = nearest_inputs()
    index, d2, ties = nearest_reference()
    assert (ties >= 2).sum() >= 20
    assert (d2 == 0).sum() >= 1000 and np.isin(np.arange(N_QUERY), ids).sum() >= 1000


def test_nearest_numpy_equals_brute_force():
    _, src, query = nearest_inputs()
    index, d2, _ = nearest_reference()
    got, got_d2 = RS.nearest_index_numpy(src, query, return_dist=True)
    assert got.dtype == np.int64 and np.array_equal(got, index) and np.array_equal(got_d2, d2)


def test_nearest_numpy_max_dist():
    _, src, query = nearest_inputs()
    index, d2, _ = nearest_reference()
    far = d2 > 0.03 * 0.03
    assert 100 <= far.sum() <= N_QUERY - 100
    got, got_d2 = RS.nearest_index(src, query[:2048], max_dist=0.03, return_dist=True, backend='numpy')
    assert np.array_equal(got, np.where(far, -1, index)[:2048])
    assert np.array_equal(got_d2, np.where(far, np.inf, d2)[:2048])


@pytest.mark.parametrize('name', sorted(nearest_cases()))
def test_nearest_numpy_small_cases(name):
    src, query, max_dist = nearest_cases()[name]
    index, d2, _ = brute_nearest(src, query, max_dist)
    got, got_d2 = RS.nearest_index_numpy(src, query, max_dist=max_dist, return_dist=True)
    assert np.array_equal(got, index) and np.array_equal(got_d2, d2)
    if name == 'duplicate_sources':
        assert (index[:400] == np.arange(400)).all()          # the lowest of the three copies
    if name == 'max_dist_small':
        assert (index < 0).any() and (index >= 0).any()


def test_nearest_numpy_rejects_bad_input():
    _, src, query = nearest_inputs()
    bad = query[:4].copy()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError):
        RS.nearest_index_numpy(src[:10], bad)
    with pytest.raises(ValueError):
        RS.nearest_index_numpy(bad, query[:4])
    with pytest.raises(ValueError):
        RS.nearest_index_numpy(src[:0], query[:4])
    with pytest.raises(ValueError):
        RS.nearest_index_numpy(src[:10], query[:4], max_dist=-1.0)


def test_default_cell_is_about_two_points_per_cell():
    cell = RS.nearest_default_cell([-4, -3, -1.5], [4, 3, 1.5], 17500)
    assert cell == (2 * 8.0 * 6.0 * 3.0 / 17500) ** (1 / 3)
    assert RS.nearest_default_cell([0, 0, 0], [2, 2, 0], 800) == (2 * 4.0 / 800) ** 0.5          # a flat cloud
    assert RS.nearest_default_cell([1, 1, 1], [1, 1, 1], 5) == 1.0
    assert RS.nearest_default_cell([1e9, 0, 0], [1e9 + 1, 1, 1], 10**6) == (1e9 + 1) / 2.0**29   # the range floor


# ---- masks ------------------------------------------------------------------------------------------------------------
N_SRC, N_MASKS, N_OUT = 4097, 37, 10001


@functools.lru_cache(maxsize=None)
def mask_case():
    """-> (dense bool [37, 4097], index int64 [10001] with repeats and -1)"""
    rng = np.random.default_rng(23)
    density = np.linspace(0.0, 1.0, N_MASKS)
    dense = rng.random((N_MASKS, N_SRC)) < density[:, None]
    dense[0] = False
    dense[-1] = True
    runs = rng.random((N_MASKS, N_SRC)) < 0.02                   # long runs next to the salt and pepper
    dense[1:-1:3] = (np.cumsum(runs[1:-1:3], 1) % 2).astype(bool)
    index = rng.integers(-1, N_SRC, size=N_OUT)
    index[:3] = [N_SRC - 1, 0, -1]
    index[-40:] = N_SRC - 1                                      # the last word ends inside a run of the full mask
    assert (index < 0).sum() >= 1 and np.unique(index).size < index.size
    return dense, index


def packed_rows(dense):
    n, length = dense.shape
    out = np.zeros((n, (length + 31) // 32 * 4), np.uint8)
    p = np.packbits(dense, axis=1, bitorder='little')
    out[:, :p.shape[1]] = p
    return out


def gathered(dense, index):
    out = dense[:, np.maximum(index, 0)].copy()
    out[:, index < 0] = False
    return out


def runs_of(dense):
    """np.diff runs of every row -> (starts, ends, bounds)"""
    starts, ends, bounds = [], [], [0]
    for row in dense:
        e = np.diff(np.concatenate([[0], row.astype(np.int8), [0]]))
        starts.append(np.flatnonzero(e == 1))
        ends.append(np.flatnonzero(e == -1))
        bounds.append(bounds[-1] + starts[-1].size)
    return np.concatenate(starts), np.concatenate(ends), np.array(bounds, np.int64)


def test_mask_bits_gather_numpy():
    dense, index = mask_case()
    got = RS.mask_bits_gather(packed_rows(dense), N_SRC, index)
    want = gathered(dense, index)
    assert got.shape == (N_MASKS, (N_OUT + 31) // 32 * 4)
    bits = np.unpackbits(got, axis=1, bitorder='little')
    assert np.array_equal(bits[:, :N_OUT].astype(bool), want) and not bits[:, N_OUT:].any()
    with pytest.raises(ValueError):
        RS.mask_bits_gather_numpy(packed_rows(dense), N_SRC, np.array([0, N_SRC]))


def test_mask_runs_from_bits_numpy():
    dense, index = mask_case()
    for d in (dense, gathered(dense, index)):
        assert not d[0].any()                                    # an all-zeros row
        if d.shape[1] == N_OUT:
            assert np.array_equal(d[-1], index >= 0)             # all ones but for the -1 holes
        else:
            assert d[-1].all()                                   # an all-ones row
        starts, ends, bounds = RS.mask_runs_from_bits(packed_rows(d), d.shape[1])
        s, e, b = runs_of(d)
        assert np.array_equal(starts, s) and np.array_equal(ends, e) and np.array_equal(bounds, b)
        assert starts.dtype == ends.dtype == np.int32 and bounds.dtype == np.int64
    tail = packed_rows(dense[:, :100])
    tail[:, 12] |= 0xF0                                          # bits at and beyond n_points are ignored
    s, e, b = runs_of(dense[:, :100])
    got = RS.mask_runs_from_bits_numpy(tail, 100)
    assert np.array_equal(got[0], s) and np.array_equal(got[1], e) and np.array_equal(got[2], b)


# ---- propagate_result ------------------------------------------------------------------------------------------------
def instance_list(dense, scan_id='scene0'):
    rng = np.random.default_rng(5)
    return [dict(scan_id=scan_id, label_id=int(rng.integers(1, 19)), conf=float(rng.random()), pred_mask=rle_encode(m))
            for m in dense.astype(np.uint8)]


def round_trip(backend):
    dense, index = mask_case()
    insts = instance_list(dense)
    out = propagate_result(dict(scan_id='scene0', pred_instances=insts), index, backend=backend)
    assert len(out['pred_instances']) == N_MASKS
    for got, inst in zip(out['pred_instances'], insts):
        want = rle_decode(inst['pred_mask']).astype(bool)[np.maximum(index, 0)] & (index >= 0)
        assert got['pred_mask']['length'] == N_OUT
        assert np.array_equal(rle_decode(got['pred_mask']).astype(bool), want)
        assert got['pred_mask'] == rle_encode(want.astype(np.uint8))          # canonical: maximal runs, 1-based
        assert (got['scan_id'], got['label_id'], got['conf']) == (inst['scan_id'], inst['label_id'], inst['conf'])
    assert out['pred_instances'][0]['pred_mask']['counts'] == ''             # the empty mask stays in the list
    return out


def test_mask_round_trip_through_propagate_result():
    round_trip('numpy')


N_E2E = 20001


@functools.lru_cache(maxsize=None)
def e2e_case():
    """a synthetic result over the voxel-thinned cloud + everything of the full cloud"""
    xyz = cloud()[:N_E2E]
    ids, inverse, _ = brute_voxels(xyz, 0.1, 'center')
    n = ids.size
    rng = np.random.default_rng(31)
    lab = rng.integers(0, 6, n)
    result = dict(scan_id='scene1', coords_float=xyz[ids], semantic_preds=rng.integers(0, 20, n),
                  offset_preds=rng.normal(size=(n, 3)).astype(np.float32),
                  panoptic_preds=rng.integers(1, 2**20, n).astype(np.uint32),
                  semantic_labels=rng.integers(0, 20, n), instance_labels=lab,
                  offset_labels=np.zeros((n, 3), np.float32),
                  pred_instances=instance_list(np.stack([lab == k for k in range(6)])))
    gt = dict(semantic_labels=np.arange(N_E2E) % 20, instance_labels=np.arange(N_E2E) % 7)
    return xyz, ids, inverse, result, gt


def check_e2e(out, result_before):
    xyz, ids, inverse, result, gt = e2e_case()
    assert np.array_equal(out['semantic_preds'], result['semantic_preds'][inverse])
    assert np.array_equal(out['offset_preds'], result['offset_preds'][inverse])
    assert np.array_equal(out['panoptic_preds'], result['panoptic_preds'][inverse])
    assert out['panoptic_preds'].dtype == np.uint32 and out['offset_preds'].dtype == np.float32
    assert out['coords_float'] is xyz and out['scan_id'] == 'scene1'
    assert out['semantic_labels'] is gt['semantic_labels'] and out['instance_labels'] is gt['instance_labels']
    assert 'offset_labels' not in out                             # not in gt: dropped, never gathered
    for got, inst in zip(out['pred_instances'], result['pred_instances']):
        assert got['pred_mask']['length'] == N_E2E and got['label_id'] == inst['label_id']
        assert np.array_equal(rle_decode(got['pred_mask']), rle_decode(inst['pred_mask'])[inverse])
    # the input is untouched
    assert set(result) == set(result_before)
    for k, v in result_before.items():
        assert result[k] is v
    assert all(i['pred_mask']['length'] == ids.size for i in result['pred_instances'])


def test_propagate_result_end_to_end():
    xyz, ids, inverse, result, gt = e2e_case()
    out = propagate_result(result, inverse, coords=xyz, gt=gt, backend='numpy')
    check_e2e(out, dict(result))
    # without coords and gt: the thinned coordinates and labels are dropped
    bare = propagate_result(result, torch.from_numpy(inverse), backend='numpy')
    assert 'coords_float' not in bare and 'semantic_labels' not in bare and 'instance_labels' not in bare
    # -1: ignore_label, zeros, cleared bits
    holes = inverse.copy()
    holes[::3] = -1
    out = propagate_result(result, holes, ignore_label=-7, backend='numpy')
    assert (out['semantic_preds'][::3] == -7).all() and not out['offset_preds'][::3].any()
    assert not out['panoptic_preds'][::3].any()
    assert np.array_equal(out['semantic_preds'][1::3], result['semantic_preds'][inverse][1::3])
    assert not rle_decode(out['pred_instances'][2]['pred_mask'])[::3].any()
    with pytest.raises(ValueError):
        propagate_result(result, np.array([0, ids.size]), backend='numpy')
    with pytest.raises(ValueError):
        propagate_result(result, inverse, backend='cpu')


def test_propagate_result_resolves_lazy_results():
    from concurrent.futures import Future

    from softgroup_amd.util.lazy import LazyResults
    xyz, ids, inverse, result, gt = e2e_case()
    lazy = LazyResults(scan_id='scene1', semantic_preds=result['semantic_preds'])
    fut = Future()
    fut.set_result(dict(pred_instances=result['pred_instances']))
    lazy.defer(fut)
    out = propagate_result(lazy, inverse, backend='numpy')
    assert type(out) is dict and len(out['pred_instances']) == 6
    assert np.array_equal(out['semantic_preds'], result['semantic_preds'][inverse])


# ---- command line ----------------------------------------------------------------------------------------------------
def load_cli():
    spec = importlib.util.spec_from_file_location('sg_tools_downsample', os.path.join(ROOT, 'tools', 'downsample.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def write_rooms(data_dir):
    os.makedirs(data_dir)
    rooms = {}
    for k, n in enumerate([1500, 777]):
        rng = np.random.default_rng(k)
        scene = f'Area_{k + 1}_office_{k}'
        room = (cloud()[k * 2000:k * 2000 + n].copy(), rng.integers(0, 256, (n, 3)).astype(np.uint8),
                rng.integers(0, 13, n).astype(np.int64), rng.integers(-1, 9, n).astype(np.int64) * 100 - 100,
                k, scene)
        torch.save(room, os.path.join(data_dir, f'{scene}_inst_nostuff.pth'))
        rooms[scene] = room
    return rooms


def check_room(path, room, ids):
    got = torch.load(path, weights_only=False)
    assert len(got) == 6 and got[4] == room[4] and got[5] == room[5]
    for g, r in zip(got[:4], room[:4]):
        assert isinstance(g, np.ndarray) and g.dtype == r.dtype and np.array_equal(g, r[ids])


def test_cli_random_sample_and_voxel_grid(tmp_path):
    cli = load_cli()
    data_dir = str(tmp_path / 'preprocess')
    rooms = write_rooms(data_dir)
    assert cli.main(['--data-dir', data_dir, '--ratio', '0.25', '--seed', '0', '--backend', 'numpy']) == 2
    for scene, room in rooms.items():
        n = room[0].shape[0]
        path = os.path.join(data_dir + '_sample', f'{scene}_inst_nostuff.pth')
        check_room(path, room, np.array(random.Random(0).sample(range(n), int(n * 0.25))))
    stamp = {f: os.stat(os.path.join(data_dir + '_sample', f)).st_mtime_ns for f in os.listdir(data_dir + '_sample')}
    assert cli.main(['--data-dir', data_dir, '--ratio', '0.5', '--seed', '1', '--backend', 'numpy']) == 0      # all skipped
    assert stamp == {f: os.stat(os.path.join(data_dir + '_sample', f)).st_mtime_ns for f in stamp}
    assert cli.main(['--data-dir', data_dir, '--voxel-size', '0.25', '--pick', 'first', '--backend', 'numpy',
                     '--verbose']) == 2
    for scene, room in rooms.items():
        path = os.path.join(data_dir + '_voxelize', f'{scene}_inst_nostuff.pth')
        check_room(path, room, brute_voxels(room[0], 0.25, 'first')[0])
    assert cli.main(['--data-dir', data_dir, '--voxel-size', '0.25', '--backend', 'numpy']) == 0


def test_cli_reports_and_keeps_extra_tuple_entries(tmp_path, capsys):
    """the tuple is handled as a sequence: four per-point arrays are thinned, whatever follows is carried over"""
    cli = load_cli()
    data_dir = str(tmp_path / 'rooms')
    rooms = write_rooms(data_dir)
    assert cli.main(['--data-dir', data_dir, '--ratio', '0.1', '--seed', '3', '--verbose']) == 2
    text = capsys.readouterr().out
    for scene, room in rooms.items():
        n = room[0].shape[0]
        assert f'{scene}: {n} -> {int(n * 0.1)} points' in text
    assert cli.main(['--data-dir', data_dir, '--ratio', '0.1', '--seed', '3', '--verbose']) == 0
    assert capsys.readouterr().out.count('skipped') == 2


def test_propagate_result_takes_any_integer_index_and_no_other(tmp_path):
    xyz, ids, inverse, result, gt = e2e_case()
    want = propagate_result(result, inverse, backend='numpy')
    for index in (inverse.astype(np.int32), torch.from_numpy(inverse).int(), inverse.tolist()):
        got = propagate_result(result, index, backend='numpy')
        assert np.array_equal(got['semantic_preds'], want['semantic_preds'])
        assert got['pred_instances'] == want['pred_instances']
    for index in (inverse.astype(np.float32), torch.from_numpy(inverse).double(), inverse.reshape(1, -1), inverse > 0):
        with pytest.raises(ValueError):
            propagate_result(result, index, backend='numpy')
    with pytest.raises(ValueError):
        propagate_result(result, np.array([0, -2]), backend='numpy')


def test_mask_runs_supported_is_the_range_of_the_library():
    assert RS.mask_runs_supported(300, 1_000_000) and RS.mask_runs_supported(0, 0)
    assert RS.mask_runs_supported(1, 2**31 - 1) and not RS.mask_runs_supported(1, 2**31)
    assert not RS.mask_runs_supported(1000, 5_000_000)            # 1000 * 2.5 M runs: beyond int32 run numbers
    assert RS.mask_runs_supported(858, 5_000_000) and not RS.mask_runs_supported(859, 5_000_000)
