"""The training-time transform on the device (train_data.hip) against the reference (golden file of
tests/golden/make_ref_train_data.py), against the numpy restatement at full size, stage by stage through the
C ABI, in rng='device' mode, and end to end into forward_train."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'golden'))

from softgroup_amd import _lib as L  # noqa: E402
from softgroup_amd import data, synthetic  # noqa: E402
from softgroup_amd.data import TrainTransform, collate_train_device  # noqa: E402
from softgroup_amd.data.train import blur_numpy, interp_numpy  # noqa: E402
from test_train_data import TOL, as_np, assert_item, gold, raw_inputs, run_case  # noqa: E402
from train_data_cases import CASES, NAMES  # noqa: E402

pytestmark = pytest.mark.gpu

SCANNET_CFG = dict(scale=50, spatial_shape=[128, 512], max_npoint=250000, min_npoint=5000)
KITTI_CFG = dict(scale=20, spatial_shape=[128, 512], max_npoint=80000, min_npoint=5000)


@pytest.mark.parametrize('case', [c for c in CASES if not c.get('batch')], ids=lambda c: c['name'])
def test_device_numpy_stream_equals_reference_item(case):
    g = gold()
    items = run_case(g, case, device='cuda')
    for j, item in enumerate(items):
        if item is not None:
            assert item[1].is_cuda and item[9].is_cuda
        assert_item(g, case['name'], j, item)


def test_device_batch_equals_reference_collate_fn():
    g = gold()
    case = [c for c in CASES if c.get('batch')][0]
    batch = collate_train_device(run_case(g, case, device='cuda'), min_spatial=case['voxel_cfg']['spatial_shape'][0])
    for k, v in batch.items():
        ref = g[f'batch_batch_{k}']
        got = as_np(v) if k != 'scan_ids' else np.asarray(v)
        if k == 'scan_ids':
            assert list(got) == list(ref)
            continue
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        if k in ('coords_float', 'pt_offset_labels'):
            np.testing.assert_allclose(got, ref, rtol=0, atol=1e-5 if k == 'pt_offset_labels' else 1e-6, err_msg=k)
        else:
            assert np.array_equal(got, ref), k
    assert batch['coords'].dtype == torch.int64 and batch['instance_pointnum'].dtype == torch.int32
    assert batch['feats'].dtype == torch.float32 and batch['batch_idxs'].dtype == torch.int32


def _kitti_like(n=120000, seed=3):
    xyz, rgb, inst = synthetic.scene_s2(seed=seed, n=n, room_scale=1.0)
    things, stuff = [10, 11, 15, 18, 30], [40, 48, 50, 70, 71, 80, 0, 1]
    cls = np.where(inst >= 0, np.array(things)[np.clip(inst, 0, None) % 5], np.array(stuff)[np.arange(n) % 8])
    word = (np.where(inst >= 0, inst * 7 + 3, 0).astype(np.int64) << 16 | cls).astype(np.int32)
    from train_data_cases import KITTI_MAP
    sem, lab = data.kitti_labels(word, dict(KITTI_MAP))
    return (xyz * 3).astype(np.float32), rgb[:, :1].copy(), sem, lab


def _scannet(n=150000, seed=1):
    xyz, rgb, inst = synthetic.scene_s2(seed=seed, n=n)
    sem = np.where(inst >= 0, 2 + inst % 18, 0).astype(np.float64)
    return xyz, rgb, sem, inst.astype(np.float64)


def _compare(a, b):
    assert (a is None) == (b is None)
    if a is None:
        return
    for k, x, y in zip(NAMES[1:], a[1:], b[1:]):
        x, y = as_np(x), as_np(y)
        assert x.shape == y.shape, (k, x.shape, y.shape)
        if k in TOL:
            np.testing.assert_allclose(x, y, rtol=0, atol=TOL[k], err_msg=k)
        else:
            assert np.array_equal(x, y), k


@pytest.mark.parametrize('which', ['scannet', 'kitti'])
def test_device_equals_numpy_restatement_at_size(which):
    raw, cfg, ds = (_scannet(), SCANNET_CFG, 'scannetv2') if which == 'scannet' else (_kitti_like(), KITTI_CFG, 'kitti')
    out = []
    for dev in ('cpu', 'cuda'):
        np.random.seed(7)
        torch.manual_seed(7)
        out.append(TrainTransform(cfg, dataset=ds, rng='numpy', device=dev)(*raw))
    _compare(*out)
    if which == 'kitti':          # the crop iterated
        assert cfg['min_npoint'] <= out[1][1].shape[0] <= cfg['max_npoint'] < raw[0].shape[0]


def _keys(a):
    return a.view(np.int64).view(np.uint64)


def test_blur_and_elastic_stages_through_the_c_abi():
    lib = L.lib()
    rng = np.random.default_rng(0)
    bb = (23, 17, 9)
    grids = rng.standard_normal((3, ) + bb).astype(np.float32)
    d = torch.from_numpy(grids).cuda()
    tmp = torch.empty_like(d)
    L.check(lib.sg_train_blur(L.ptr(d), L.ptr(tmp), *bb, 3, L.stream()), 'sg_train_blur')
    got = d.cpu().numpy()
    ref = np.stack([blur_numpy(x) for x in grids])
    ulp = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    assert ulp.max() <= 1, ulp.max()
    gran, mag = 6, 40.0
    half = np.array([(b - 1) * gran for b in bb], np.float64)
    x = rng.uniform(-1.05, 1.05, (20000, 3)) * half        # (some points outside the grid: g = 0 there)
    x[:64] = np.round(x[:64] / 12) * 12                     # nodes
    dx = torch.from_numpy(x.copy()).cuda()
    stats = torch.empty(9, dtype=torch.int64, device='cuda')
    L.check(lib.sg_train_elastic(L.ptr(dx), x.shape[0], L.ptr(torch.from_numpy(ref).cuda()), *bb, float(gran), mag,
                                 L.ptr(stats), L.stream()), 'sg_train_elastic')
    g = np.stack([interp_numpy(r, gran, x) for r in ref], 1)
    np.testing.assert_allclose((dx.cpu().numpy() - x) / mag, g, rtol=0, atol=1e-12)
    want = x + g * mag
    assert np.abs(dx.cpu().numpy() - want).max() <= 1e-12 * np.abs(want).max()
    from softgroup_amd.data._train_device import _decode
    h = _decode(stats.cpu().numpy())
    assert np.array_equal(h[0:3], np.abs(dx.cpu().numpy()).max(0)) and np.array_equal(h[3:6], dx.cpu().numpy().min(0))


def test_device_grid_blur_std():
    """a device-drawn N(0,1) grid blurred by the six passes: interior std (19/81)^(3/2) ~ 0.114"""
    lib = L.lib()
    gen = torch.Generator(device='cuda')
    gen.manual_seed(5)
    d = torch.randn(1, 64, 64, 64, generator=gen, device='cuda')
    tmp = torch.empty_like(d)
    L.check(lib.sg_train_blur(L.ptr(d), L.ptr(tmp), 64, 64, 64, 1, L.stream()), 'sg_train_blur')
    s = float(d[0, 4:-4, 4:-4, 4:-4].std())
    assert abs(s - (19 / 81) ** 1.5) < 0.004, s


@pytest.mark.parametrize('which', ['scannet', 'kitti'])
def test_device_rng_is_repeatable_and_keeps_the_invariants(which):
    raw, cfg, ds = (_scannet(), SCANNET_CFG, 'scannetv2') if which == 'scannet' else (_kitti_like(), KITTI_CFG, 'kitti')
    tf = TrainTransform(cfg, dataset=ds, rng='device', seed=123)
    a, b = tf(*raw, index=4), tf(*raw, index=4)
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(as_np(x), as_np(y))
    other = tf(*raw, index=5)
    assert not np.array_equal(as_np(a[2]), as_np(other[2])) if a[2].shape == other[2].shape else True
    _, coord, cf, feat, sem, inst, k, pointnum, cls, off = a
    n = coord.shape[0]
    assert cfg['min_npoint'] <= n <= cfg['max_npoint']
    c = as_np(coord)
    assert c.min() >= 0 and (c.max(0) < cfg['spatial_shape'][1]).all()
    lab = as_np(inst)
    ids = np.unique(lab[lab != -100])
    assert np.array_equal(ids, np.arange(k))
    pn = as_np(pointnum)
    assert pn.sum() == (lab != -100).sum() and (pn > 0).all()
    cfn = as_np(cf)
    mean = np.stack([cfn[lab == i].mean(0) for i in range(k)]).astype(np.float32)
    want = np.where((lab >= 0)[:, None], mean[np.clip(lab, 0, None)], np.float32(-100)) - cfn
    np.testing.assert_allclose(as_np(off), want, rtol=0, atol=1e-5)


def test_forward_train_from_device_batches_and_prefetch_equality():
    from softgroup_amd.model import SoftGroup
    import copy
    tf = TrainTransform(SCANNET_CFG, dataset='scannetv2', rng='device', seed=9)
    scans = [_scannet(seed=s) for s in (1, 2, 3, 4)]

    def make(batch, device='cuda'):
        return collate_train_device([tf(*s, scan_id=f'scan{i}', index=i) for i, s in batch], device=device)

    inline = make(list(enumerate(scans)))
    assert inline['batch_size'] == 4 and inline['coords'].shape[0] > 4 * 100000
    torch.manual_seed(0)
    model = SoftGroup(**copy.deepcopy(synthetic.SCANNET_MODEL_CFG)).cuda()
    with torch.no_grad():
        model.semantic_linear[-1].weight.normal_(0, 20.0)
    model.train()
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    loss, log_vars = model(inline, return_loss=True)
    assert torch.isfinite(loss) and all(np.isfinite(float(v)) for v in log_vars.values())
    opt.zero_grad()
    loss.backward()
    opt.step()
    batches = [list(enumerate(scans))[:2], list(enumerate(scans))[2:]]
    got = list(data.prefetch_device(batches, collate=make, workers=2))
    ref = [make(b) for b in batches]
    assert len(got) == 2
    for x, y in zip(got, ref):
        for k in y:
            if isinstance(y[k], torch.Tensor):
                assert torch.equal(x[k], y[k]), k
            else:
                assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), k
