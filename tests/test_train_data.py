"""The training-time transform against the REFERENCE'S OWN dataset classes run with training=True
(tests/golden/ref_train_data.npz, made by tests/golden/make_ref_train_data.py).  CPU part:
``TrainTransform(device='cpu', rng='numpy')`` replays the reference's random stream and must give the
reference's item -- exact fields exactly, coord_float within 1e-9, pt_offset_label within 1e-5.  The device
path is checked in tests/test_train_data_gpu.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))

from softgroup_amd.data import TrainTransform  # noqa: E402
from train_data_cases import CASES, NAMES, raw_case, raw_digest  # noqa: E402

GOLD = os.path.join(HERE, 'golden', 'ref_train_data.npz')
TOL = {'coord_float': 1e-9, 'pt_offset_label': 1e-5}


def gold():
    return np.load(GOLD)


def raw_inputs(g, case, j):
    load = raw_case(case, j)['load']
    assert str(g[f"{case['name']}_raw{j}_sha256"]) == raw_digest(load), 'regenerated scan differs from the golden input'
    return tuple(load[k] for k in ('xyz', 'rgb', 'sem', 'inst'))


def transform(case, device='cpu'):
    return TrainTransform(case['voxel_cfg'], dataset=case['dataset'], aug_prob=case['aug_prob'],
                          x4_split=case.get('x4_split', False), rng='numpy', device=device)


def run_case(g, case, device='cpu'):
    """our items for every seed of a case, the global streams seeded as the generator seeded them"""
    tf = transform(case, device)
    out = []
    for j, seed in enumerate(case['seeds']):
        np.random.seed(seed)
        torch.manual_seed(seed)
        out.append(tf(*raw_inputs(g, case, j), scan_id=f'scene{j:04d}_00', index=j))
    return out


def as_np(v):
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().numpy()
    return np.asarray(v)


def assert_item(g, name, j, item):
    assert bool(g[f'{name}_item{j}_none']) == (item is None), (name, j)
    if item is None:
        return
    for k, v in zip(NAMES[1:], item[1:]):
        ref, got = g[f'{name}_item{j}_{k}'], as_np(v)
        assert got.shape == ref.shape, (name, j, k, got.shape, ref.shape)
        if k in TOL:
            np.testing.assert_allclose(got, ref, rtol=0, atol=TOL[k], err_msg=f'{name} {j} {k}')
        else:
            assert np.array_equal(got, ref), (name, j, k)


def test_cases_in_the_golden_file_are_the_ones_here():
    assert json.loads(str(gold()['cases'])) == json.loads(json.dumps(CASES))


@pytest.mark.parametrize('case', [c for c in CASES if not c.get('batch')], ids=lambda c: c['name'])
def test_cpu_transform_equals_reference_item(case):
    g = gold()
    items = run_case(g, case)
    for j, item in enumerate(items):
        assert_item(g, case['name'], j, item)
    if case['name'] == 'scannet_none':
        assert items == [None]
    if case['name'] == 'scannet_crop':
        assert items[0][1].shape[0] < raw_inputs(g, case, 0)[0].shape[0]


def test_cpu_transform_batch_case_equals_reference_collate_entries():
    """the two items of the batch case against the per-point entries of the reference collate_fn's batch"""
    g = gold()
    case = [c for c in CASES if c.get('batch')][0]
    items = run_case(g, case)
    b = lambda k: g[f"batch_batch_{k}"]   # noqa: E731
    assert np.array_equal(np.concatenate([as_np(it[1]) for it in items]), b('coords')[:, 1:])
    np.testing.assert_allclose(np.concatenate([as_np(it[2]) for it in items]).astype(np.float32),
                               b('coords_float'), rtol=0, atol=1e-6)
    assert np.array_equal(np.concatenate([as_np(it[3]) for it in items]), b('feats'))
    assert np.array_equal(np.concatenate([as_np(it[4]) for it in items]), b('semantic_labels'))
    shift = np.where(as_np(items[1][5]) != -100, as_np(items[1][5]) + items[0][6], -100)
    assert np.array_equal(np.concatenate([as_np(items[0][5]), shift]), b('instance_labels'))
    assert np.array_equal(np.concatenate([it[7] for it in items]), b('instance_pointnum'))
    assert np.array_equal(np.concatenate([it[8] for it in items]), b('instance_cls'))
    np.testing.assert_allclose(np.concatenate([as_np(it[9]) for it in items]).astype(np.float32),
                               b('pt_offset_labels'), rtol=0, atol=1e-5)


def test_aug_half_takes_both_branches_and_the_stream_advances_like_the_reference():
    """aug_prob=0.5: one seed with the elastic passes, one without; afterwards the global stream sits exactly
    where the reference's left it (the next draw is the reference's next draw)"""
    g = gold()
    case = [c for c in CASES if c['name'] == 'scannet_aug_half'][0]
    tf = transform(case)
    seen = []
    for j, seed in enumerate(case['seeds']):
        tf.trace = []
        np.random.seed(seed)
        torch.manual_seed(seed)
        tf(*raw_inputs(g, case, j))
        seen.append(any(t[0] == 'elastic' for t in tf.trace))
    assert sorted(seen) == [False, True]


def test_blur_and_interp_restatements_on_edge_values():
    from softgroup_amd.data.train import blur_numpy, interp_numpy
    grid = np.zeros((3, 4, 5), np.float32)
    grid[1, 2, 3] = 81
    out = blur_numpy(grid)
    assert out.dtype == np.float32 and out.shape == grid.shape
    assert abs(out[1, 2, 3] - 81 * (3 / 9) ** 3) < 1e-3 and (out >= 0).all()   # (the centre: 3 of 9 taps per axis)
    # at a node the interpolation returns the node value; outside the grid 0
    g = np.arange(60, dtype=np.float32).reshape(3, 4, 5)
    x = np.array([[-12.0, -18.0, -24.0], [0.0, 6.0, 0.0], [12.0, 18.0, 24.0], [13.0, 0, 0]])
    v = interp_numpy(g, 6, x)
    assert v[0] == g[0, 0, 0] and v[2] == g[2, 3, 4] and v[3] == 0


def test_from_config_presets():
    vc = dict(scale=50, spatial_shape=[128, 512], max_npoint=250000, min_npoint=5000)
    tf = TrainTransform.from_config(dict(type='s3dis', voxel_cfg=vc, x4_split=True), device='cpu', rng='numpy')
    assert tf.x4_split and tf.preset['step'] == 64 and tf.preset['cls_shift'] == 0
    tf = TrainTransform.from_config(dict(type='kitti', voxel_cfg=vc), device='cpu')
    assert tf.preset['down'] == 5 and tf.preset['relabel'] == 'rank' and tf.preset['cls_shift'] == 11
    with pytest.raises(ValueError):
        TrainTransform(vc, dataset='nope', device='cpu')
