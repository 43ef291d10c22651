"""The test-time transform on the device (TestTransform, train_data.hip) against the reference's own items and
batches (tests/golden/ref_collate*.npz), against ``scan_item`` at the bench sizes and on label edge cases, into
``forward_test``, under ``prefetch_device``, run to run, and on its fallbacks."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from softgroup_amd import _lib as L  # noqa: E402
from softgroup_amd import data, synthetic  # noqa: E402
from softgroup_amd.data import (TestTransform, TrainTransform, collate_device, collate_train_device,  # noqa: E402
                                collate_x4_test_device, scan_item)
from test_data_golden import GOLD, VARIANTS  # noqa: E402
from test_test_data import (as_np, assert_item, blobs, fixture_scans, kitti_words, kitti_yaml_map,  # noqa: E402
                            labelled, voxel_cfg)
from test_train_data import TOL  # noqa: E402

pytestmark = pytest.mark.gpu

BATCH_TOL = {'coords_float': 1e-6, 'pt_offset_labels': 1e-5}


def transforms(dataset, **kw):
    vc = voxel_cfg(dataset)
    return TestTransform(vc, dataset=dataset, **kw), TestTransform(vc, dataset=dataset, device='cpu', **kw)


def assert_device_item(item):
    for v in item:
        if isinstance(v, torch.Tensor):
            assert v.is_cuda
    assert isinstance(item[7], torch.Tensor) and isinstance(item[8], torch.Tensor)


def assert_batch(batch, g, prefix):
    keys = [k[len(prefix):] for k in g.files if k.startswith(prefix)]
    assert set(keys) == set(batch.keys())
    for k in keys:
        ref, got = g[prefix + k], batch[k]
        if isinstance(got, torch.Tensor):
            assert got.is_cuda, k
        got = as_np(got)
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        if ref.dtype.kind in 'fiu':
            assert got.dtype == ref.dtype, (k, got.dtype, ref.dtype)
        if k in BATCH_TOL:
            np.testing.assert_allclose(got, ref, rtol=0, atol=BATCH_TOL[k], err_msg=k)
        else:
            assert np.array_equal(got, ref), k


# ---- reference fixtures ------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', fixture_scans(), ids=lambda c: c[0])
def test_device_item_equals_reference_item(case):
    name, tkw, call, ref = case
    item = TestTransform(voxel_cfg(tkw['dataset']), **tkw)(**call)
    assert_device_item(item)
    assert_item(item, ref, TOL, name)


def test_device_batches_equal_reference_collate_fn():
    cases = {c[0]: c for c in fixture_scans()}
    tf = TestTransform(voxel_cfg('scannetv2'))
    batch = collate_train_device([tf(**cases[f'scannet{i}'][2]) for i in range(2)], min_spatial=128)
    assert_batch(batch, np.load(GOLD), 'batch_')
    tf = TestTransform(voxel_cfg('s3dis'), dataset='s3dis', x4_split=True)
    batch = collate_x4_test_device([tf(**cases['s3dis'][2])], min_spatial=128)
    assert_batch(batch, np.load(VARIANTS), 's3dis_batch_')
    # the collate= form: the same dicts
    again = tf.collate([cases['s3dis'][2]])
    for k, v in batch.items():
        assert (torch.equal(v, again[k]) if isinstance(v, torch.Tensor) else np.array_equal(v, again[k])), k


# ---- at size against scan_item -----------------------------------------------------------------------------
def _scans():
    out = {}
    xyz, rgb, inst = blobs(150000, 40, 1)
    out['scannet_150k'] = ('scannetv2', {}, (xyz, rgb) + labelled(inst, 2))
    xyz, rgb, inst = blobs(600000, 300, 2, extent=(50.0, 50.0, 10.0))
    out['stpls3d_600k'] = ('stpls3d', {}, (xyz, rgb) + labelled(inst, 1, n_cls=14))
    xyz, rgb, inst = blobs(1000003, 40, 4, extent=(10.0, 8.0, 3.0))      # (n % 4 == 3)
    out['s3dis_x4_1m'] = ('s3dis', dict(x4_split=True), (xyz, rgb) + labelled(inst, 0, n_cls=13))
    xyz, rgb, inst = blobs(50000, 0, 5)
    out['all_unlabelled'] = ('scannetv2', {}, (xyz, rgb) + labelled(inst, 2))
    out['with_label_false'] = ('scannetv2', {}, (xyz, rgb, np.zeros(50000), np.zeros(50000)))
    out['with_label_false_kitti'] = ('kitti', {}, (xyz, rgb[:, :1], np.zeros(50000), np.zeros(50000)))
    xyz, rgb, inst = blobs(80000, 30, 6)
    gaps = np.asarray([0, 2, 3, 7, 8, 11, 12, 13, 20, 21, 25, 29, 33, 40, 41, 47, 52, 60, 61, 70, 72, 80, 90, 95, 99,
                       100, 120, 150, 151, 200])
    inst = np.where(inst >= 0, gaps[np.clip(inst, 0, None)], -100)
    out['id_gaps'] = ('scannetv2', {}, (xyz, rgb) + labelled(inst, 2))
    out['x4_id_gaps_int32'] = ('s3dis', dict(x4_split=True),
                               (xyz, rgb, labelled(inst, 0)[0].astype(np.int32), inst.astype(np.int32)))
    return out


SCANS = _scans()


@pytest.mark.parametrize('name', list(SCANS))
def test_device_item_equals_scan_item_at_size(name):
    ds, kw, args = SCANS[name]
    dev, cpu = transforms(ds, **kw)
    got = dev(*args, scan_id=name)
    assert_device_item(got)
    assert_item(got, cpu(*args, scan_id=name), TOL, name)
    if name == 'id_gaps':
        assert got[6] == 30 and set(np.unique(as_np(got[5]))) == set(range(30)) | {-100}


def test_kitti_raw_words_at_size_and_train_transform_keyword():
    xyz, rem, words = kitti_words()
    dev, cpu = transforms('kitti', learning_map=kitti_yaml_map())
    got = dev(xyz, rem, label_words=words, scan_id='k')
    assert_item(got, cpu(xyz, rem, label_words=words, scan_id='k'), TOL, 'kitti')
    assert got[6] == 30 and (words < 0).any()
    # the decode alone against kitti_labels; a labelled first point makes the ranked labels int64
    sem, lab = data.kitti_labels(words, kitti_yaml_map())
    first = int(np.argmax(lab != -100))
    w2 = np.roll(words, -first)
    assert_item(dev(np.roll(xyz, -first, 0), np.roll(rem, -first, 0), label_words=w2),
                cpu(np.roll(xyz, -first, 0), np.roll(rem, -first, 0), label_words=w2), TOL, 'kitti first labelled')
    # TrainTransform: label_words= equals the decoded labels, item for item
    vc = dict(scale=20, spatial_shape=[128, 512], max_npoint=80000, min_npoint=5000)
    tw = TrainTransform(vc, dataset='kitti', rng='device', seed=4, learning_map=kitti_yaml_map())
    a, b = tw(xyz, rem, label_words=words, index=2), tw(xyz, rem, sem, lab, index=2)
    assert (a is None) == (b is None)
    for x, y in zip(a[1:] if a else (), b[1:] if b else ()):
        assert np.array_equal(as_np(x), as_np(y))


# ---- model output, prefetching, repeatability ----------------------------------------------------------------
def _scene(seed, n=20000):
    xyz, rgb, inst = synthetic.scene_s2(seed=seed, n=n, room_scale=0.37)
    return (xyz, rgb) + labelled(inst, 2) + (f's{seed}', )


def test_forward_test_on_device_batch_equals_host_items():
    tf = TestTransform(voxel_cfg('scannetv2'))
    model = synthetic.build_model(seed=0)
    model.async_results = False
    scans = [_scene(5), _scene(6)]
    with torch.no_grad():
        a = dict(model(tf.collate(scans)))
        b = dict(model(collate_device([scan_item(*s[:4], scale=50, scan_id=s[4]) for s in scans])))
    assert len(a['pred_instances']) == len(b['pred_instances']) > 0
    for x, y in zip(a['pred_instances'], b['pred_instances']):
        assert x['label_id'] == y['label_id'] and x['conf'] == y['conf'] and x['pred_mask'] == y['pred_mask']
    np.testing.assert_array_equal(a['semantic_preds'], b['semantic_preds'])


def _equal_batches(x, y):
    assert x.keys() == y.keys()
    for k in y:
        if isinstance(y[k], torch.Tensor):
            assert torch.equal(x[k], y[k]), k
        else:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), k


def test_prefetch_batches_equal_serial_and_runs_repeat():
    tf = TestTransform(voxel_cfg('scannetv2'))
    batches = [[_scene(s, 30000 + 1000 * s) for s in (1, 2)], [_scene(3)], [_scene(s) for s in (4, 5, 6)]]
    serial = [tf.collate(b) for b in batches]
    got = list(data.prefetch_device(batches, collate=tf.collate, workers=2))
    assert len(got) == 3
    for x, y in zip(got, serial):
        _equal_batches(x, y)
    for ds, kw, args in (SCANS['scannet_150k'], SCANS['s3dis_x4_1m']):
        tf = TestTransform(voxel_cfg(ds), dataset=ds, **kw)
        a, b = tf(*args), tf(*args)
        for x, y in zip(a[1:], b[1:]):
            assert np.array_equal(as_np(x), as_np(y))
            if isinstance(x, torch.Tensor) and x.dtype == torch.float64:
                assert np.array_equal(as_np(x).view(np.int64), as_np(y).view(np.int64))


# ---- fallbacks -----------------------------------------------------------------------------------------------
def test_fallbacks():
    xyz, rgb, inst = blobs(9001, 12, 8)
    sem, inst = labelled(inst, 2)
    for kw, ds in ((dict(), 'scannetv2'), (dict(x4_split=True), 's3dis')):
        dev, cpu = transforms(ds, **kw)
        bad = xyz.copy()
        bad[17, 1] = np.nan
        bad[4000, 2] = np.inf
        got = dev(bad, rgb, sem, inst)
        assert_device_item(got)
        assert_item(got, cpu(bad, rgb, sem, inst), where=f'non-finite {ds}')
        with pytest.raises(ValueError):
            dev(xyz[:0], rgb[:0], sem[:0], inst[:0])
    with pytest.raises(ValueError):
        transforms('s3dis', x4_split=True)[0](xyz[:3], rgb[:3], sem[:3], inst[:3])
    # a key missing from the learning map: the reference's KeyError, test and train transform
    xyz, rem, words = kitti_words(30000, 10)
    m = kitti_yaml_map()
    words = words.copy()
    words[12345] = (words[12345] & ~0xFFFF) | 99
    dev = TestTransform(voxel_cfg('kitti'), dataset='kitti', learning_map=m)
    with pytest.raises(KeyError) as e:
        dev(xyz, rem, label_words=words)
    assert e.value.args[0] == 99
    with pytest.raises(KeyError):
        TrainTransform(dict(scale=20, spatial_shape=[128, 512], max_npoint=80000, min_npoint=5000), dataset='kitti',
                       learning_map=m)(xyz, rem, label_words=words)
    # more than 8192 instance ids
    xyz, rgb, _ = blobs(20000, 0, 9)
    ids = np.arange(20000, dtype=np.float64) % 9000
    with pytest.raises(L.SoftGroupHipError):
        TestTransform(voxel_cfg('scannetv2'))(xyz, rgb, ids % 18, ids)
