"""The HIP kernels of csrc/resample.hip and the device paths on top of them, on the inputs and against the
brute-force references of tests/test_resample.py: equality everywhere, two calls give equal bytes."""
import os
import sys

import numpy as np
import pytest
import torch

from softgroup_amd import _lib as L
from softgroup_amd import synthetic
from softgroup_amd.data import random_downsample, voxel_downsample
from softgroup_amd.ops import nms as MN
from softgroup_amd.ops import resample as RS
from softgroup_amd.util import propagate_result, results as R, rle_decode

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_resample import (BAD_CLOUDS, CELLS, EDGE_N, MIN_TIES, N, N_MASKS, N_OUT, N_QUERY, N_SRC, PICKS,  # noqa: E402
                           VOXELS, brute_nearest, brute_voxels, check_e2e, check_voxels, cloud, e2e_case, edge_cloud,
                           gathered, mask_case, nearest_cases, nearest_inputs, nearest_reference, packed_rows, round_trip,
                           runs_of, voxel_reference)

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared inputs are read-only)


# ---- voxels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pick', PICKS)
@pytest.mark.parametrize('voxel', VOXELS)
def test_voxel_downsample_device_equals_brute_force(voxel, pick):
    ref = voxel_reference(voxel, pick)
    if pick == 'center' and voxel in MIN_TIES:
        assert ref[2] >= MIN_TIES[voxel]
    xyz = dev(cloud())
    ids, inverse = voxel_downsample(xyz, voxel, pick=pick, backend='device')
    assert ids.is_cuda and inverse.is_cuda
    check_voxels(ids.cpu().numpy(), inverse.cpu().numpy(), ref)
    ids2, inverse2 = RS.grid_downsample(xyz, voxel, pick)          # the same bytes, the kernel's own int32
    assert ids2.dtype == inverse2.dtype == torch.int32
    assert torch.equal(ids2.long(), ids) and torch.equal(inverse2.long(), inverse)


@pytest.mark.parametrize('pick', PICKS)
@pytest.mark.parametrize('n', EDGE_N + [64])
def test_voxel_downsample_device_edge_sizes(n, pick):
    x = edge_cloud(n)
    ids, inverse = voxel_downsample(dev(x).reshape(n, 3), 0.25, pick=pick, backend='device')
    check_voxels(ids.cpu().numpy(), inverse.cpu().numpy(), brute_voxels(x, 0.25, pick))
    got = voxel_downsample(x, 0.25, pick=pick, backend='device')          # numpy in, numpy out
    assert isinstance(got[0], np.ndarray) and np.array_equal(got[0], ids.cpu().numpy())


@pytest.mark.parametrize('name', sorted(BAD_CLOUDS))
def test_voxel_downsample_device_rejects_invalid_points(name):
    x, voxel = BAD_CLOUDS[name]
    with pytest.raises(ValueError):
        voxel_downsample(dev(x), voxel, backend='device')
    big = cloud()[:5000].copy()          # one invalid point among many: still no result
    big[4321] = x[1]
    with pytest.raises(ValueError):
        voxel_downsample(dev(big), voxel, backend='device')


def test_random_downsample_device():
    a, b = random_downsample(10001, 0.25, seed=5, rng='device'), random_downsample(10001, 0.25, seed=5, rng='device')
    assert a.is_cuda and a.dtype == torch.int64 and a.numel() == 2500 and torch.equal(a, b)
    assert a.unique().numel() == 2500 and 0 <= int(a.min()) and int(a.max()) < 10001


# ---- nearest point ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cell', CELLS)
def test_nearest_device_equals_brute_force(cell):
    _, src, query = nearest_inputs()
    index, d2, ties = nearest_reference()
    assert (ties >= 2).sum() >= 20 and (d2 == 0).sum() >= 1000
    got, got_d2, scanned = RS.nearest_index(dev(src), dev(query), cell=cell, return_dist=True, return_meta=True)
    assert got.is_cuda and got.dtype == torch.int64 and got_d2.dtype == torch.float64
    assert np.array_equal(got.cpu().numpy(), index)
    assert np.array_equal(got_d2.cpu().numpy(), d2)               # equal to the bit
    if cell is None:
        assert scanned < N_QUERY // 4                             # the grid answers, the scan is the exception
        again = RS.nearest_index(dev(src), dev(query))
        assert torch.equal(again, got)
    if cell == 1e-3:
        assert scanned > N_QUERY // 2                             # cells far smaller than the spacing: the scan answers


def test_nearest_device_max_dist():
    _, src, query = nearest_inputs()
    index, d2, _ = nearest_reference()
    far = d2 > 0.03 * 0.03
    assert 100 <= far.sum() <= N_QUERY - 100
    got, got_d2 = RS.nearest_index(dev(src), dev(query), max_dist=0.03, return_dist=True)
    assert np.array_equal(got.cpu().numpy(), np.where(far, -1, index))
    assert np.array_equal(got_d2.cpu().numpy(), np.where(far, np.inf, d2))
    host = RS.nearest_index(src, query, max_dist=0.03, backend='device')          # numpy in, numpy out, through the device
    assert isinstance(host, np.ndarray) and host.dtype == np.int64 and np.array_equal(host, np.where(far, -1, index))


@pytest.mark.parametrize('cell', [None, 0.05])
@pytest.mark.parametrize('name', sorted(nearest_cases()))
def test_nearest_device_small_cases(name, cell):
    src, query, max_dist = nearest_cases()[name]
    index, d2, _ = brute_nearest(src, query, max_dist)
    got, got_d2, scanned = RS.nearest_index(dev(src), dev(query).reshape(-1, 3), cell=cell, max_dist=max_dist,
                                            return_dist=True, return_meta=True)
    assert np.array_equal(got.cpu().numpy(), index) and np.array_equal(got_d2.cpu().numpy(), d2)
    if name == 'two_clusters':
        assert scanned >= 200          # the queries in the gap cost a scan each, not a walk
    if name == 'far_queries':
        assert scanned >= 64
    if name == 'duplicate_sources':
        assert (index[:400] == np.arange(400)).all()
    if name == 'max_dist_small':
        assert (index < 0).any() and (index >= 0).any()


def test_nearest_device_rejects_bad_input():
    _, src, query = nearest_inputs()
    bad = query[:300].copy()
    bad[222, 1] = np.nan
    with pytest.raises(ValueError):
        RS.nearest_index(dev(src[:1000]), dev(bad))
    with pytest.raises(ValueError):
        RS.nearest_index(dev(bad), dev(query[:10]), cell=0.1)
    with pytest.raises(ValueError):
        RS.nearest_index(dev(src[:0]).reshape(0, 3), dev(query[:4]))
    # a cell so small that the grid is out of range: not an error, every query takes the scan
    index, _, _ = brute_nearest(src[:1000], query[:300])
    got, scanned = RS.nearest_index(dev(src[:1000]), dev(query[:300]), cell=1e-12, return_meta=True)
    assert np.array_equal(got.cpu().numpy(), index) and scanned == 300


# ---- masks ------------------------------------------------------------------------------------------------------------
def bit_rows(dense):
    return dev(packed_rows(dense).view(np.int32))


def test_mask_bits_gather_device():
    dense, index = mask_case()
    got = RS.mask_bits_gather(bit_rows(dense), N_SRC, dev(index))
    assert got.is_cuda and got.dtype == torch.int32 and got.shape == (N_MASKS, (N_OUT + 31) // 32)
    bits = np.unpackbits(got.cpu().numpy().view(np.uint8), axis=1, bitorder='little')
    assert np.array_equal(bits[:, :N_OUT].astype(bool), gathered(dense, index))
    assert not bits[:, N_OUT:].any()                              # the tail bits of the last word
    assert np.array_equal(got.cpu().numpy().view(np.uint8), RS.mask_bits_gather_numpy(packed_rows(dense), N_SRC, index))


def test_mask_bits_gather_flags_an_index_beyond_the_source():
    dense, index = mask_case()
    lib = L.lib()
    bad = index.copy()
    bad[[5, 7000]] = [N_SRC, 2**31 - 1]
    want = gathered(dense, np.where(bad >= N_SRC, -1, bad))
    bits, d_idx = bit_rows(dense), dev(bad.astype(np.int32))
    out = torch.full((N_MASKS, (N_OUT + 31) // 32), -1, dtype=torch.int32, device='cuda')
    meta = torch.full((1, ), 7, dtype=torch.int32, device='cuda')
    L.check(lib.sg_mask_bits_gather(L.ptr(bits), N_MASKS, N_SRC, L.ptr(d_idx), N_OUT, L.ptr(out), L.ptr(meta),
                                    L.stream()), 'sg_mask_bits_gather')
    got = np.unpackbits(out.cpu().numpy().view(np.uint8), axis=1, bitorder='little')
    assert int(meta.item()) == 1 and np.array_equal(got[:, :N_OUT].astype(bool), want) and not got[:, N_OUT:].any()
    L.check(lib.sg_mask_bits_gather(L.ptr(bits), N_MASKS, N_SRC, L.ptr(dev(index.astype(np.int32))), N_OUT, L.ptr(out),
                                    L.ptr(meta), L.stream()), 'sg_mask_bits_gather')
    assert int(meta.item()) == 0


def test_mask_runs_from_bits_device():
    dense, index = mask_case()
    for d in (dense, gathered(dense, index), dense[:, :100], dense[:0], dense[:, :0]):
        n_points = d.shape[1]
        rows = packed_rows(d)
        if n_points == 100:
            rows[:, 12] |= 0xF0                                   # bits at and beyond n_points are ignored
        starts, ends, bounds = RS.mask_runs_from_bits(dev(rows.view(np.int32)), n_points)
        s, e, b = runs_of(d) if d.size else (np.zeros(0), np.zeros(0), np.zeros(d.shape[0] + 1))
        assert starts.dtype == ends.dtype == torch.int32 and bounds.dtype == torch.int64
        assert np.array_equal(starts.cpu().numpy(), s) and np.array_equal(ends.cpu().numpy(), e)
        assert np.array_equal(bounds.cpu().numpy(), b)
        if d.size:                                                # ... and they are what the expansion takes
            back = MN.mask_bits_from_runs(starts, ends, bounds, n_points)
            got = np.unpackbits(back.cpu().numpy().view(np.uint8), axis=1, bitorder='little')[:, :n_points]
            assert np.array_equal(got.astype(bool), d)


def test_mask_round_trip_device_equals_numpy():
    a, b = round_trip('device'), round_trip('numpy')
    assert [i['pred_mask'] for i in a['pred_instances']] == [i['pred_mask'] for i in b['pred_instances']]


def test_propagate_result_device_rejects_unsorted_runs():
    dense, index = mask_case()
    insts = [dict(scan_id='s', label_id=1, conf=0.5, pred_mask=dict(length=N_SRC, counts='9 2 1 3'))]
    with pytest.raises(ValueError):
        propagate_result(dict(scan_id='s', pred_instances=insts), index, backend='device')
    want = propagate_result(dict(scan_id='s', pred_instances=insts), index, backend='numpy')
    assert rle_decode(want['pred_instances'][0]['pred_mask']).sum() > 0


# ---- propagate_result ------------------------------------------------------------------------------------------------
def test_propagate_result_end_to_end_device():
    xyz, ids, inverse, result, gt = e2e_case()
    got_ids, got_inverse = voxel_downsample(dev(xyz), 0.1, backend='device')
    assert np.array_equal(got_ids.cpu().numpy(), ids)
    out = propagate_result(result, got_inverse, coords=xyz, gt=gt, backend='device')
    check_e2e(out, dict(result))
    ref = propagate_result(result, inverse, coords=xyz, gt=gt, backend='numpy')
    assert [i['pred_mask'] for i in out['pred_instances']] == [i['pred_mask'] for i in ref['pred_instances']]


def test_scan_of_a_thinned_scene_propagated_and_saved(tmp_path):
    """a ScanForward result of a 20 k-point scene carried to 4x the points by the nearest thinned point"""
    xyz, rgb, inst = synthetic.scene_s2(seed=5, n=20000, room_scale=0.37)
    batch = synthetic.make_batch(xyz, rgb, instance_labels=inst)
    model = synthetic.build_model(seed=0)
    with torch.no_grad():
        res = model(batch)
    assert getattr(model.__dict__.get('_scan_forward'), 'last', None) is not None, 'the one-call path must have run'
    rng = np.random.default_rng(3)
    n_full = 4 * xyz.shape[0]
    full = np.repeat(np.asarray(xyz, np.float32), 4, axis=0)
    full[1::4] += rng.normal(0, 0.002, (xyz.shape[0], 3)).astype(np.float32)
    full[2::4] += rng.normal(0, 0.002, (xyz.shape[0], 3)).astype(np.float32)
    full[3::4] += rng.normal(0, 0.002, (xyz.shape[0], 3)).astype(np.float32)
    index = RS.nearest_index(dev(np.asarray(xyz, np.float32)), dev(full))
    want, _, _ = brute_nearest(np.asarray(xyz, np.float32), full[:2048])
    assert np.array_equal(index[:2048].cpu().numpy(), want) and int(index.min()) >= 0
    gt = dict(semantic_labels=np.zeros(n_full, np.int64), instance_labels=np.full(n_full, -100, np.int64),
              offset_labels=np.zeros((n_full, 3), np.float32), color_feats=np.zeros((n_full, 3), np.float32),
              gt_instances=np.zeros(n_full, np.int64))
    preds = res['pred_instances']
    assert len(preds) > 0
    out = propagate_result(res, index, coords=full, gt=gt, backend='device')
    idx = index.cpu().numpy()
    assert np.array_equal(out['semantic_preds'], np.asarray(res['semantic_preds'])[idx])
    assert len(out['pred_instances']) == len(preds)
    for g, p in zip(out['pred_instances'][:8], preds[:8]):
        assert g['pred_mask']['length'] == n_full
        assert np.array_equal(rle_decode(g['pred_mask']), rle_decode(p['pred_mask'])[idx])

    class Dataset:
        NYU_ID = (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39)

    tasks = synthetic.SCANNET_MODEL_CFG['test_cfg']['eval_tasks']
    R.save_results(str(tmp_path), [out], tasks, Dataset, backend='device')
    got = R.load_pred_instances(str(tmp_path / 'pred_instance'), out['scan_id'], backend='device')
    assert len(got) == len(preds)
    for g, p in zip(got[:8], out['pred_instances'][:8]):
        assert g['pred_mask'].shape[0] == n_full and np.array_equal(g['pred_mask'], rle_decode(p['pred_mask']).astype(bool))
    assert np.load(str(tmp_path / 'semantic_pred' / f"{out['scan_id']}.npy")).shape[0] == n_full
    assert np.load(str(tmp_path / 'coords' / f"{out['scan_id']}.npy")).shape == (n_full, 3)


# ---- the caller's errors and where the index lives -------------------------------------------------------------------
def test_nearest_query_with_a_bad_source_writes_minus_one_and_scans_nothing():
    """a source coordinate that is not finite is an error the Python layer raises for: the kernels must not first
    spend n_src * n_query work on it -- every index is -1 at once and the work list stays empty"""
    _, src, query = nearest_inputs()
    bad = src[:2000].copy()
    bad[1234, 2] = np.inf
    lib = L.lib()
    d_src, d_query = dev(bad), dev(query[:1000])
    n_src, n_query, cell = 2000, 1000, 0.1
    grid = torch.empty(lib.sg_nearest_grid_bytes(n_src), dtype=torch.uint8, device='cuda')
    meta = torch.full((2, ), 9, dtype=torch.int32, device='cuda')
    L.check(lib.sg_nearest_build(L.ptr(d_src), n_src, cell, L.ptr(grid), grid.numel(), L.ptr(meta), L.stream()),
            'sg_nearest_build')
    index = torch.full((n_query, ), 7, dtype=torch.int32, device='cuda')
    dist2 = torch.zeros(n_query, dtype=torch.float64, device='cuda')
    ws = torch.empty(lib.sg_nearest_query_workspace_bytes(n_query), dtype=torch.uint8, device='cuda')
    L.check(lib.sg_nearest_query(L.ptr(d_src), n_src, cell, L.ptr(grid), grid.numel(), L.ptr(d_query), n_query, -1.0,
                                 L.ptr(index), L.ptr(dist2), L.ptr(meta), L.ptr(ws), ws.numel(), L.stream()),
            'sg_nearest_query')
    assert meta.cpu().tolist() == [0, 1]                          # nothing on the work list; the source flag
    assert (index == -1).all() and torch.isinf(dist2).all()


def test_mask_bits_gather_check_raises_like_the_numpy_path():
    dense, index = mask_case()
    bad = index.copy()
    bad[77] = N_SRC
    bits = bit_rows(dense)
    with pytest.raises(ValueError):
        RS.mask_bits_gather(bits, N_SRC, dev(bad), check=True)
    with pytest.raises(ValueError):
        RS.mask_bits_gather_numpy(packed_rows(dense), N_SRC, bad)
    quiet = RS.mask_bits_gather(bits, N_SRC, dev(bad))            # the default: counts as -1, nothing synchronises
    assert torch.equal(quiet, RS.mask_bits_gather(bits, N_SRC, dev(np.where(bad >= N_SRC, -1, bad))))
    assert torch.equal(RS.mask_bits_gather(bits, N_SRC, dev(index), check=True), RS.mask_bits_gather(bits, N_SRC, dev(index)))


def test_propagate_result_keeps_a_device_index_on_the_device(monkeypatch):
    from softgroup_amd.util import propagate as P
    xyz, ids, inverse, result, gt = e2e_case()
    holes = inverse.copy()
    holes[::5] = -1
    want = propagate_result(result, holes, backend='numpy')
    on_dev = {k: (dev(v) if k in ('semantic_preds', 'offset_preds') else v) for k, v in result.items()
              if k != 'panoptic_preds'}                           # (uint32: numpy only)

    def no_host(self):
        raise AssertionError('a CUDA index was brought to the host')

    monkeypatch.setattr(P._Index, 'host', no_host)
    out = propagate_result(on_dev, dev(holes), backend='device')
    assert out['semantic_preds'].is_cuda and out['offset_preds'].is_cuda
    assert np.array_equal(out['semantic_preds'].cpu().numpy(), want['semantic_preds'])
    assert np.array_equal(out['offset_preds'].cpu().numpy(), want['offset_preds'])
    assert [i['pred_mask'] for i in out['pred_instances']] == [i['pred_mask'] for i in want['pred_instances']]
    with pytest.raises(ValueError):
        propagate_result(on_dev, dev(np.array([0, ids.size])), backend='device')


def test_propagate_result_auto_takes_numpy_beyond_the_device_range(monkeypatch):
    """n_inst * ceil(N_full / 2) >= 2**31 is far too large for a test: the range answer is replaced, the route is
    the real one"""
    from softgroup_amd.util import propagate as P
    dense, index = mask_case()
    result = dict(scan_id='s', pred_instances=[dict(scan_id='s', label_id=1, conf=0.5, pred_mask=m)
                                               for m in (dense[3], dense[20])])
    want = propagate_result(result, index, backend='numpy')
    monkeypatch.setattr(RS, 'mask_runs_supported', lambda n, n_points: False)
    monkeypatch.setattr(P, '_masks_device', lambda *a: pytest.fail('the device route was taken'))
    got = propagate_result(result, index, backend='auto')
    assert got['pred_instances'] == want['pred_instances']
    monkeypatch.undo()
    assert propagate_result(result, index, backend='auto')['pred_instances'] == want['pred_instances']
