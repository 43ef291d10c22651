"""Masks cut into connected components on the device: ``sg_mask_split_count`` / ``_fill`` through ctypes, the Python
surface and the model's ``get_instances`` paths plus ``ScanForward``, against the brute force and the numpy twin of
tests/test_mask_split.py.  Equality everywhere; the reference has no such step."""
import os
import sys

import numpy as np
import pytest
import torch

from softgroup_amd import _lib as L
from softgroup_amd import ops, synthetic
from softgroup_amd.ops import split as MS
from softgroup_amd.util import nms_instances, split_instances
from softgroup_amd.util import split as US

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_mask_split import (HAND, RADIUS, R, SHAPES, bits_of, chain_case, check_hand, dense_of,  # noqa: E402
                             instance_list, reference, same_as_brute, same_lists)

pytestmark = pytest.mark.gpu

_MODE = {'split': 0, 'largest': 1}
POISON = 0x5A5A5A5A
SPARE = 3               # rows behind the expected outputs that must stay untouched


def pairs_of(bits, N):
    return int(dense_of(bits, N).sum())


def run_count(bits, N, xyz, radius, min_npoint=1, mode='split', ws_pairs=None):
    """the count pass on host arrays -> (rc, meta list, state for run_fill)"""
    lib = L.lib()
    dev = torch.device('cuda')
    n = bits.shape[0]
    d_bits = torch.from_numpy(np.array(bits, dtype=np.int32)).to(dev)
    d_xyz = torch.from_numpy(np.array(xyz, dtype=np.float32)).to(dev)
    meta = torch.full((4, ), -77, dtype=torch.int32, device=dev)
    nb = lib.sg_mask_split_workspace_bytes(n, N, pairs_of(bits, N) if ws_pairs is None else ws_pairs)
    assert nb > 0
    ws = torch.full((nb, ), 0x5A, dtype=torch.uint8, device=dev)
    rc = lib.sg_mask_split_count(L.ptr(d_xyz), d_bits.data_ptr() if d_bits.numel() else None, n, N, float(radius),
                                 min_npoint, _MODE[mode], L.ptr(meta), L.ptr(ws), nb, L.stream())
    torch.cuda.synchronize()
    return rc, meta.cpu().tolist(), (n, N, ws, d_bits, d_xyz)


def run_fill(state, meta, capacity=None):
    """the fill pass into poisoned buffers -> (out_bits, source, npoint) as numpy, SPARE rows behind the outputs"""
    lib = L.lib()
    n, N, ws, _, _ = state
    dev = ws.device
    words = (N + 31) // 32
    n_out = meta[0]
    capacity = n_out if capacity is None else capacity
    out_bits = torch.full((n_out + SPARE, words), POISON, dtype=torch.int32, device=dev)
    source = torch.full((n_out + SPARE, ), POISON, dtype=torch.int32, device=dev)
    npoint = torch.full((n_out + SPARE, ), POISON, dtype=torch.int32, device=dev)
    L.check(lib.sg_mask_split_fill(n, N, meta[2], L.ptr(ws), ws.numel(), capacity, L.ptr(out_bits), L.ptr(source),
                                   L.ptr(npoint), L.stream()), 'sg_mask_split_fill')
    torch.cuda.synchronize()
    return out_bits.cpu().numpy(), source.cpu().numpy(), npoint.cpu().numpy()


def run_kernel(bits, N, xyz, radius, min_npoint=1, mode='split'):
    """both passes -> (out_bits, source, npoint, meta); a validity flag raises ValueError as the Python surface does;
    every word of the outputs is written and nothing behind them is"""
    rc, meta, state = run_count(bits, N, xyz, radius, min_npoint, mode)
    L.check(rc, 'sg_mask_split_count')
    if meta[1] & 3:
        assert meta[0] == 0
        raise ValueError('invalid coordinate of a mask point')
    assert meta[1] == 0, f'flags {meta[1]}'
    assert meta[2] == pairs_of(bits, N)
    out_bits, source, npoint = run_fill(state, meta)
    n_out = meta[0]
    for a in (out_bits, source, npoint):
        assert (a[n_out:] == POISON).all(), 'written behind the outputs'
    return out_bits[:n_out], source[:n_out], npoint[:n_out], meta


def kernel3(*args):
    return run_kernel(*args)[:3]


# ---- the kernels --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(HAND))
def test_kernel_hand_made_cases(name):
    check_hand(name, kernel3)


@pytest.mark.parametrize('mode,min_npoint', [('split', 1), ('largest', 1), ('split', 12)])
@pytest.mark.parametrize('n,N', SHAPES)
def test_kernel_equals_brute_force(n, N, mode, min_npoint):
    xyz, dense, want = reference(n, N, min_npoint, mode)
    out_bits, source, npoint, meta = run_kernel(bits_of(dense), N, xyz, RADIUS, min_npoint, mode)
    same_as_brute((out_bits, source, npoint), want, N)
    assert meta[3] == len(reference(n, N)[2][1])            # components before the selection


def big_case():
    """64 masks over 20 000 points, about 3 000 points each: more pairs than one grid stride of the per-pair
    kernels (8192 x 256 threads is above it, 2048 x 256 of the per-word kernel is not) and many occupied cells"""
    n, N = 64, 20000
    rng = np.random.default_rng(11)
    side = (N * (4.0 / 3.0) * np.pi * RADIUS ** 3 / 10.0) ** (1.0 / 3.0)
    xyz = ((rng.random((N, 3)) - 0.5) * side).astype(np.float32)
    rho = side * (0.085 * 3.0 / (4.0 * np.pi)) ** (1.0 / 3.0)
    dense = np.zeros((n, N), bool)
    for k in range(n):
        for _ in range(2):
            c = (rng.random(3) - 0.5) * (side - 2 * rho)
            dense[k] |= ((xyz.astype(np.float64) - c) ** 2).sum(1) <= rho * rho
        dense[k, rng.integers(N, size=20)] = True
    return xyz, dense


def test_kernel_equals_twin_on_200k_pairs():
    xyz, dense = big_case()
    N = dense.shape[1]
    bits = bits_of(dense)
    assert 150000 <= pairs_of(bits, N) <= 260000
    want = MS.mask_components_numpy(bits, N, xyz, RADIUS, 3, 'split')
    assert len(want[1]) > 64
    out_bits, source, npoint, _ = run_kernel(bits, N, xyz, RADIUS, 3, 'split')
    assert np.array_equal(out_bits, want[0]) and np.array_equal(source, want[1]) and np.array_equal(npoint, want[2])


def test_fill_respects_capacity():
    n, N = 67, 2049
    xyz, dense, want = reference(n, N)
    rc, meta, state = run_count(bits_of(dense), N, xyz, RADIUS)
    assert rc == 0 and meta[0] == len(want[1]) > 8 and meta[1] == 0
    cap = meta[0] - 5
    out_bits, source, npoint = run_fill(state, meta, capacity=cap)
    same_as_brute((out_bits[:cap], source[:cap], npoint[:cap]), tuple(w[:cap] for w in want), N)
    for a in (out_bits, source, npoint):
        assert (a[cap:] == POISON).all(), 'written beyond the capacity'
    # a capacity above the number of outputs writes the outputs only
    out_bits, source, npoint = run_fill(state, meta, capacity=meta[0] + 2)
    same_as_brute((out_bits[:meta[0]], source[:meta[0]], npoint[:meta[0]]), want, N)
    assert (out_bits[meta[0]:] == POISON).all() and (source[meta[0]:] == POISON).all()


def test_workspace_too_small_reports_the_pairs():
    n, N = 67, 2049
    xyz, dense, want = reference(n, N)
    bits = bits_of(dense)
    P = pairs_of(bits, N)
    lib = L.lib()
    assert lib.sg_mask_split_workspace_bytes(n, N, P // 4) < lib.sg_mask_split_workspace_bytes(n, N, P)
    rc, meta, _ = run_count(bits, N, xyz, RADIUS, ws_pairs=P // 4)
    assert rc == -2 and b'workspace' in lib.sg_last_error() and meta[2] == P and meta[0] == 0
    # the Python surface starts from a guess (a few masks' worth of the cloud) and asks again with the count
    n, N = 40, 4096
    assert n * N > 4 * N + 65536
    pts = np.zeros((N, 3), np.float32)
    pts[:, 0] = np.arange(N) * R
    every = torch.from_numpy(bits_of(np.ones((n, N), bool))).cuda()
    out = ops.mask_components(every, N, torch.from_numpy(pts).cuda(), R)
    assert out[1].cpu().tolist() == list(range(n)) and out[2].cpu().tolist() == [N] * n
    assert torch.equal(out[0], every)


@pytest.mark.parametrize('shuffle', [None, 4], ids=['in_order', 'shuffled'])
def test_chain_longer_than_any_round_count(shuffle):
    xyz, dense = chain_case(shuffle=shuffle)
    out_bits, source, npoint, meta = run_kernel(bits_of(dense), 3000, xyz, R)
    assert source.tolist() == [0] and npoint.tolist() == [3000] and meta[3] == 1
    assert np.array_equal(out_bits, bits_of(dense))
    xyz, dense = chain_case(cut=1500, shuffle=shuffle)
    out_bits, source, npoint, meta = run_kernel(bits_of(dense), 3000, xyz, R)
    assert source.tolist() == [0, 0] and sorted(npoint.tolist()) == [1499, 1500] and meta[3] == 2
    pos = np.rint(xyz[:, 1] / R).astype(np.int64) + 1000
    rows = dense_of(out_bits, 3000)
    assert np.flatnonzero(rows[0])[0] < np.flatnonzero(rows[1])[0]      # ascending key
    low, high = (rows[0], rows[1]) if rows[0][np.flatnonzero(pos == 0)[0]] else (rows[1], rows[0])
    assert np.array_equal(low, pos < 1500) and np.array_equal(high, pos > 1500)


def test_dense_cell_is_one_component():
    """2000 points inside one cell, all within the radius of each other: the quadratic loop over the cell ends with
    the loop-bound flag clear"""
    N = 2000
    rng = np.random.default_rng(2)
    xyz = (0.01 + 0.12 * rng.random((N, 3))).astype(np.float32)       # diameter 0.21 < 0.25, cell [0, 0.25)^3
    dense = np.ones((1, N), bool)
    out_bits, source, npoint, meta = run_kernel(bits_of(dense), N, xyz, R)
    assert meta == [1, 0, N, 1] and source.tolist() == [0] and npoint.tolist() == [N]
    assert np.array_equal(out_bits, bits_of(dense))


def test_two_calls_give_the_same_bytes():
    n, N = 300, 4097
    xyz, dense, _ = reference(n, N)
    a = run_kernel(bits_of(dense), N, xyz, RADIUS, 2, 'largest')
    b = run_kernel(bits_of(dense), N, xyz, RADIUS, 2, 'largest')
    assert a[3] == b[3]
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()


def test_range_and_arguments():
    lib = L.lib()
    assert lib.sg_mask_split_workspace_bytes(16385, 100, 10) == 0
    assert lib.sg_mask_split_workspace_bytes(4, 2 ** 31, 10) == 0
    assert lib.sg_mask_split_workspace_bytes(4, 100, 2 ** 31) == 0
    assert lib.sg_mask_split_workspace_bytes(16384, 2 ** 20, 2 ** 20) > 0
    one = torch.zeros(64, dtype=torch.int32, device='cuda')
    rc = lib.sg_mask_split_count(one.data_ptr(), one.data_ptr(), 16385, 32, 0.1, 1, 0, one.data_ptr(), one.data_ptr(),
                                 256, L.stream())
    assert rc == -4 and b'range' in lib.sg_last_error()
    rc = lib.sg_mask_split_fill(16385, 32, 1, one.data_ptr(), 256, 1, one.data_ptr(), one.data_ptr(), one.data_ptr(),
                                L.stream())
    assert rc == -4
    torch.cuda.synchronize()
    assert int(one.abs().sum()) == 0                        # no launch: nothing was written
    for radius, min_npoint, mode in ((0.0, 1, 0), (float('nan'), 1, 0), (1e200, 1, 0), (0.1, 0, 0), (0.1, 1, 2)):
        rc = lib.sg_mask_split_count(one.data_ptr(), one.data_ptr(), 1, 32, radius, min_npoint, mode, one.data_ptr(),
                                     one.data_ptr(), 256, L.stream())
        assert rc == -1


def test_invalid_coordinate_sets_the_flag():
    c = HAND['nan_in_a_mask']
    rc, meta, _ = run_count(c['bits'], c['N'], c['xyz'], c['radius'])
    assert rc == 0 and meta[0] == 0 and meta[1] == 1 and meta[3] == 0
    c = HAND['cell_out_of_range']
    rc, meta, _ = run_count(c['bits'], c['N'], c['xyz'], c['radius'])
    assert rc == 0 and meta[0] == 0 and meta[1] == 2
    with pytest.raises(ValueError):
        ops.mask_components(torch.from_numpy(c['bits']).cuda(), c['N'], torch.from_numpy(c['xyz']).cuda(), c['radius'])


# ---- Python surface -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode,min_npoint', [('split', 1), ('largest', 5)])
def test_ops_mask_components_cuda_equals_cpu(mode, min_npoint):
    n, N = 300, 4097
    xyz, dense, want = reference(n, N, min_npoint, mode)
    bits = torch.from_numpy(bits_of(dense))
    host = ops.mask_components(bits, N, torch.from_numpy(xyz), RADIUS, min_npoint, mode)
    dev = ops.mask_components(bits.cuda(), N, torch.from_numpy(xyz).cuda(), RADIUS, min_npoint, mode)
    assert all(d.is_cuda and d.dtype == torch.int32 for d in dev) and not any(h.is_cuda for h in host)
    for h, d in zip(host, dev):
        assert torch.equal(h, d.cpu())
    same_as_brute([d.cpu().numpy() for d in dev], want, N)
    # host coordinates are brought to the masks' device
    dev2 = ops.mask_components(bits.cuda(), N, xyz, RADIUS, min_npoint, mode)
    assert all(torch.equal(a, b) for a, b in zip(dev, dev2))
    none = torch.zeros((0, 129), dtype=torch.int32).cuda()
    empty = ops.mask_components(none, 4097, torch.from_numpy(xyz).cuda(), 1.0)
    assert tuple(empty[0].shape) == (0, 129) and empty[1].numel() == 0 and empty[2].numel() == 0


def _device_only(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('host path taken')
    monkeypatch.setattr(MS, 'mask_components_numpy', boom)
    monkeypatch.setattr(US, '_split_numpy', boom)


@pytest.mark.parametrize('rle', [True, False], ids=['rle', 'dense'])
@pytest.mark.parametrize('mode,min_npoint', [('split', 1), ('split', 12), ('largest', 1)])
def test_split_instances_device_equals_numpy(rle, mode, min_npoint, monkeypatch):
    n, N = 300, 4097
    xyz, dense, _ = reference(n, N)
    insts = instance_list(dense, rle)
    host = split_instances(insts, xyz, RADIUS, min_npoint, mode, backend='numpy')
    assert len(host) > 0 and (len(host) != n or mode == 'largest')      # ('largest': one output per mask)
    _device_only(monkeypatch)
    same_lists(split_instances(insts, xyz, RADIUS, min_npoint, mode, backend='device'), host)
    same_lists(split_instances(insts, torch.from_numpy(xyz).cuda(), RADIUS, min_npoint, mode, backend='device'), host)


def test_split_instances_unsorted_runs(monkeypatch):
    odd = [dict(scan_id='s', label_id=1, conf=0.5, pred_mask=dict(length=8, counts='7 2 1 2'))]
    pts = np.zeros((8, 3), np.float32)
    pts[:, 0] = np.arange(8)
    want = split_instances(odd, pts, 1.0, backend='numpy')
    assert [g['pred_mask']['counts'] for g in want] == ['1 2', '7 2']
    with pytest.raises(ValueError):
        split_instances(odd, pts, 1.0, backend='device')
    monkeypatch.setattr(US, '_AUTO', 'device')              # whatever 'auto' means: such strings take numpy
    same_lists(split_instances(odd, pts, 1.0, backend='auto'), want)


# ---- the model ----------------------------------------------------------------------------------------------------
# (the scene's surface density is ~900 points / m^2 and the untrained mask head keeps about every second point:
# at 3.5 cm the masks fall into a few components of 40 points and more, and many smaller ones that are dropped)
SPLIT = dict(radius=0.035, min_npoint=40, mode='split')
NMS = dict(thr=0.5, measure='iou', class_agnostic=True)


@pytest.fixture(scope='module')
def scene():
    xyz, rgb, inst = synthetic.scene_s2(seed=5, n=20000, room_scale=0.37)
    return synthetic.make_batch(xyz, rgb, instance_labels=inst)


def _run(model, batch, tasks, split, nms=None, scan_forward=True, native=True):
    cfg = dict(synthetic.SCANNET_MODEL_CFG['test_cfg'], eval_tasks=tasks, panoptic_skip_iou=0.5)
    if split != 'absent':
        cfg['split'] = split
    if nms is not None:
        cfg['nms'] = nms
    model.test_cfg = cfg
    model.use_scan_forward, model.use_native_scan = scan_forward, native
    with torch.no_grad():
        ret = model(batch)
    return {k: ret[k] for k in ('pred_instances', 'panoptic_preds') if k in ret}


def _want(plain, batch):
    coords = batch['coords_float'].cpu().numpy()
    out = split_instances(plain, coords, backend='numpy', **SPLIT)
    changed = len(out) != len(plain) or any(a['pred_mask'] != b['pred_mask'] for a, b in zip(out, plain))
    assert out and changed, 'the scene must have masks to cut and components to keep'
    return out


@pytest.mark.parametrize('scan_forward,native', [(True, True), (False, True), (False, False)],
                         ids=['one_call', 'staged', 'per_operator'])
def test_model_paths_split_alike(scene, scan_forward, native):
    """every path returns the numpy split of its own unsplit list; with NMS also set, NMS of that; None changes
    nothing"""
    model = synthetic.build_model(seed=0)
    tasks = ['semantic', 'instance']
    kw = dict(scan_forward=scan_forward, native=native)
    plain = _run(model, scene, tasks, 'absent', **kw)['pred_instances']
    same = _run(model, scene, tasks, None, **kw)['pred_instances']
    assert len(same) == len(plain) > 0
    for a, b in zip(same, plain):
        assert a['label_id'] == b['label_id'] and a['conf'] == b['conf'] and a['pred_mask'] == b['pred_mask']
    got = _run(model, scene, tasks, SPLIT, **kw)['pred_instances']
    if scan_forward:
        assert getattr(model.__dict__.get('_scan_forward'), 'last', None) is not None, 'the one-call path must have run'
    want = _want(plain, scene)
    same_lists(got, want)
    both = _run(model, scene, tasks, SPLIT, nms=NMS, **kw)['pred_instances']
    assert 0 < len(both) < len(want)
    same_lists(both, nms_instances(want, NMS['thr'], NMS['measure'], NMS['class_agnostic'], backend='numpy'))


@pytest.mark.parametrize('native', [True, False], ids=['device_fusion', 'host_fusion'])
def test_model_panoptic_sees_unsplit_instances(scene, native):
    model = synthetic.build_model(seed=0)
    tasks = ['semantic', 'instance', 'panoptic']
    a = _run(model, scene, tasks, 'absent', native=native)
    b = _run(model, scene, tasks, SPLIT, native=native)
    c = _run(model, scene, tasks, SPLIT, nms=NMS, native=native)
    assert np.array_equal(a['panoptic_preds'], b['panoptic_preds'])
    assert np.array_equal(a['panoptic_preds'], c['panoptic_preds'])
    want = _want(a['pred_instances'], scene)
    same_lists(b['pred_instances'], want)
    same_lists(c['pred_instances'], nms_instances(want, NMS['thr'], NMS['measure'], NMS['class_agnostic'],
                                                  backend='numpy'))
