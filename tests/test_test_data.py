"""The test-time transform (softgroup_amd.data.TestTransform) on the CPU: its presets from the dataset configs,
``device='cpu'`` (= ``scan_item``) against the REFERENCE'S OWN test-time items (tests/golden/ref_collate.npz and
ref_collate_variants.npz), and the KITTI decode table against ``kitti_labels``.  The device path is checked in
tests/test_test_data_gpu.py, which also takes its synthetic scans from here."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from softgroup_amd import data  # noqa: E402
from softgroup_amd.data import TestTransform  # noqa: E402
from test_data_golden import GOLD, NAMES, VARIANTS  # noqa: E402

VOXEL = {'scannetv2': 50, 's3dis': 50, 'stpls3d': 3, 'kitti': 20}


def voxel_cfg(dataset):
    return dict(scale=VOXEL[dataset], spatial_shape=[128, 512], max_npoint=250000, min_npoint=5000)


def kitti_map(g):
    return {int(k): int(v) for k, v in g['kitti_learning_map']}


def fixture_scans():
    """(name, transform keywords, call arguments, reference item) for every reference item in the fixtures"""
    g = np.load(GOLD)
    out = []
    for i in range(2):
        ref = {k: g[f'item{i}_{k}'] for k in NAMES}
        out.append((f'scannet{i}', dict(dataset='scannetv2'),
                    dict(xyz=g[f'raw{i}_xyz'], rgb=g[f'raw{i}_rgb'], semantic_label=g[f'raw{i}_sem'],
                         instance_label=g[f'raw{i}_inst'], scan_id=str(ref['scan_id'])), ref))
    v = np.load(VARIANTS)
    for tag, ds, kw in (('s3dis', 's3dis', dict(x4_split=True)), ('stpls3d', 'stpls3d', {})):
        ref = {k: v[f'{tag}_item_{k}'] for k in NAMES}
        out.append((tag, dict(dataset=ds, **kw),
                    dict(xyz=v[f'{tag}_raw_xyz'], rgb=v[f'{tag}_raw_rgb'], semantic_label=v[f'{tag}_raw_sem'],
                         instance_label=v[f'{tag}_raw_inst'], scan_id=str(ref['scan_id'])), ref))
    ref = {k: v[f'kitti_item_{k}'] for k in NAMES}
    raw = v['kitti_raw_data']
    out.append(('kitti', dict(dataset='kitti', learning_map=kitti_map(v)),
                dict(xyz=raw[:, :3], rgb=raw[:, 3:], label_words=v['kitti_raw_word'], scan_id=str(ref['scan_id'])),
                ref))
    return out


def as_np(v):
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().numpy()
    return np.asarray(v)


def assert_item(got, ref, tol=None, where=''):
    """every field of an item against a reference item (a fixture dict or another item): shapes and dtypes,
    integer fields exactly, the fields in ``tol`` within their absolute tolerance"""
    tol = tol or {}
    ref = ref if isinstance(ref, dict) else dict(zip(NAMES, ref))
    for k, x in zip(NAMES, got):
        y = ref[k]
        if k == 'scan_id':
            assert str(x) == str(y), where
            continue
        x, y = as_np(x), as_np(y)
        assert x.shape == y.shape, (where, k, x.shape, y.shape)
        if y.size and y.dtype.kind in 'fiu':
            assert x.dtype == y.dtype, (where, k, x.dtype, y.dtype)
        if k in tol:
            np.testing.assert_allclose(x, y, rtol=0, atol=tol[k], err_msg=f'{where} {k}')
        else:
            assert np.array_equal(x, y, equal_nan=x.dtype.kind == 'f'), (where, k)


# ---- synthetic scans at the bench sizes --------------------------------------------------------------------
def blobs(n, n_inst, seed, unlabelled=0.4, extent=(8.0, 6.0, 3.0)):
    """n points: a share `unlabelled` uniform in a box (-100), the rest in n_inst Gaussian blobs -> xyz float32,
    rgb float32 [n, 3], instance ids int64"""
    rng = np.random.default_rng(seed)
    ext = np.asarray(extent)
    m = int(n * (1 - unlabelled)) if n_inst else 0
    inst = np.full(n, -100, np.int64)
    xyz = rng.random((n, 3)) * ext
    if m:
        ids = rng.integers(0, n_inst, m)
        ids[:n_inst] = np.arange(n_inst)            # (every id present)
        ctr = rng.random((n_inst, 3)) * ext
        xyz[:m] = ctr[ids] + rng.normal(0, 0.15, (m, 3))
        inst[:m] = ids
    perm = rng.permutation(n)
    return xyz[perm].astype(np.float32), rng.uniform(-1, 1, (n, 3)).astype(np.float32), inst[perm]


def labelled(inst, shift, n_cls=18, seed=0):
    """semantic labels as the prepared files hold them (float64): instance class for instance points, a stuff
    class for the rest; instance ids as float64"""
    rng = np.random.default_rng(seed)
    sem = np.where(inst >= 0, shift + inst % n_cls, rng.integers(0, max(shift, 1), inst.shape[0]))
    return sem.astype(np.float64), inst.astype(np.float64)


KITTI_THINGS, KITTI_STUFF = (10, 11, 15, 18, 20, 30, 31, 32), (40, 44, 48, 49, 50, 51, 70, 71, 72, 80, 81, 0, 1)


def kitti_yaml_map():
    """a semantic-kitti.yaml learning_map (raw key -> 0..19)"""
    things = dict(zip(KITTI_THINGS, range(1, 9)))
    stuff = dict(zip(KITTI_STUFF, list(range(9, 20)) + [0, 0]))
    return {**things, **stuff}


def kitti_words(n=120000, n_inst=30, seed=3):
    """a LiDAR-like scan with raw 32-bit label words: instance id << 16 | class"""
    xyz, _, inst = blobs(n, n_inst, seed, extent=(60.0, 60.0, 4.0))
    rng = np.random.default_rng(seed)
    cls = np.where(inst >= 0, np.asarray(KITTI_THINGS)[np.clip(inst, 0, None) % 8],
                   np.asarray(KITTI_STUFF)[rng.integers(0, len(KITTI_STUFF), n)])
    word = ((np.where(inst >= 0, inst * 1777 + 5, 0).astype(np.int64) << 16) | cls).astype(np.int64)
    word = word.astype(np.uint32).view(np.int32)        # (ids above 2^15: negative int32 words)
    remission = rng.random((n, 1)).astype(np.float32)
    return xyz, remission, word


# ---- tests -------------------------------------------------------------------------------------------------
def test_from_config_for_each_dataset_type():
    vc = dict(scale=50, spatial_shape=[128, 512])
    for typ, shift, relabel in (('scannetv2', 2, 'fill_gaps'), ('s3dis', 0, 'fill_gaps'), ('stpls3d', 1, 'fill_gaps'),
                                ('kitti', 11, 'rank')):
        tf = TestTransform.from_config(dict(type=typ, voxel_cfg=vc, x4_split=True), device='cpu')
        assert tf.preset['cls_shift'] == shift and tf.preset['relabel'] == relabel, typ
        assert tf.x4_split == (typ == 's3dis') and tf.scale == 50 and tf.min_spatial == 128
        assert tf.preset == data.train.PRESETS[typ]
    tf = TestTransform.from_config(dict(type='s3dis', voxel_cfg=vc), device='cpu')
    assert not tf.x4_split
    with pytest.raises(ValueError):
        TestTransform(vc, dataset='nope', device='cpu')


@pytest.mark.parametrize('case', fixture_scans(), ids=lambda c: c[0])
def test_cpu_transform_equals_reference_items(case):
    name, tkw, call, ref = case
    tf = TestTransform(voxel_cfg(tkw['dataset']), device='cpu', **tkw)
    assert_item(tf(**call), ref, where=name)


def test_kitti_lut_equals_kitti_labels():
    g = np.load(VARIANTS)
    m = kitti_map(g)
    for words in (g['kitti_raw_word'], kitti_words(20000)[2]):
        sem, lab = data.kitti_labels(words, m if words is g['kitti_raw_word'] else kitti_yaml_map())
        lut = data.kitti_lut(m if words is g['kitti_raw_word'] else kitti_yaml_map())
        got = lut[words & 0xFFFF].astype(np.int64)
        assert np.array_equal(got, sem)
        assert np.array_equal(np.where(got > 10, words, -100), lab)
    lut = data.kitti_lut(m)
    assert lut.dtype == np.int32 and lut.shape == (65536, ) and (lut == data.KITTI_NO_KEY).sum() == 65536 - len(m)


def test_cpu_edge_cases():
    tf = TestTransform(voxel_cfg('scannetv2'), device='cpu')
    with pytest.raises(ValueError):
        tf(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0), np.zeros(0))
    # with_label=False: one instance of every point, class 0 - cls_shift
    xyz, rgb, _ = blobs(500, 0, 1)
    it = tf(xyz, rgb, np.zeros(500), np.zeros(500))
    assert it[6] == 1 and it[7] == [500] and it[8] == [-2.0]
    k = TestTransform(voxel_cfg('kitti'), dataset='kitti', learning_map={0: 0, 10: 1}, device='cpu')
    with pytest.raises(KeyError):
        k(xyz, rgb[:, :1], label_words=np.full(500, 10, np.int32) | (np.arange(500) == 7) * 99)
