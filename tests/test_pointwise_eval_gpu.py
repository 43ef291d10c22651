"""The device path of the point-wise evaluators and PanopticEval (sg_eval_class_tally,
sg_eval_panoptic_segments): against the reference's outputs in pointwise_golden.json (device MAE to
1e-5 relative: fp64 sum against numpy's pairwise float32 one), against the numpy path on large
KITTI- and ScanNet-like sets (integer-derived figures bit-identical), chunked, from device tensors,
repeatable, with the numpy fallback for ids the kernels cannot pack, and end to end on a small
KITTI-shaped forward_test."""
import copy
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from softgroup_amd import synthetic
from softgroup_amd.evaluation import (PanopticEval, evaluate_offset_mae, evaluate_semantic_acc,
                                      evaluate_semantic_miou)
from softgroup_amd.evaluation import panoptic_eval as pe_mod
from softgroup_amd.evaluation import point_wise_eval as pw_mod

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'golden'))
import pointwise_cases as pc  # noqa: E402
from test_pointwise_eval import GOLD, check_panoptic, check_semantic, close  # noqa: E402

pytestmark = pytest.mark.gpu

KITTI_THING = ['car', 'bicycle', 'motorcycle', 'truck', 'other-vehicle', 'person', 'bicyclist', 'motorcyclist']
KITTI_STUFF = ['road', 'parking', 'sidewalk', 'other-ground', 'building', 'fence', 'vegetation', 'trunk',
               'terrain', 'pole', 'traffic-sign']


def _device_only(monkeypatch):
    """make a numpy fallback of PanopticEval an error: the device path must carry these inputs"""
    def boom(*a, **k):
        raise AssertionError('numpy path taken')
    monkeypatch.setattr(pe_mod.PanopticEval, '_single_numpy', boom)


@pytest.mark.parametrize('name', sorted(GOLD['semantic']))
def test_semantic_device_equals_reference(name):
    check_semantic(name, 'cuda', mae_tol=None)


@pytest.mark.parametrize('name', sorted(GOLD['panoptic']))
def test_panoptic_device_equals_reference(name, capsys, monkeypatch):
    _device_only(monkeypatch)
    check_panoptic(name, 'cuda', capsys)


@pytest.mark.parametrize('name', ['kitti', 'designed'])
def test_panoptic_device_tiny_chunks(name, capsys, monkeypatch):
    _device_only(monkeypatch)
    check_panoptic(name, 'cuda', capsys, max_chunk_points=64)


@pytest.fixture(scope='module')
def kitti_set():
    scans = [pc.kitti_like(100 + s, 120000) for s in range(8)]
    return [list(x) for x in zip(*scans)]


@pytest.fixture(scope='module')
def scannet_set():
    scans = [pc.scannet_like(200 + s, 150000) for s in range(4)]
    return [list(x) for x in zip(*scans)]


def _pan_equal(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)


def test_panoptic_large_device_equals_numpy(kitti_set, monkeypatch, capsys):
    preds, sems, insts = kitti_set
    cpu = PanopticEval(KITTI_THING, KITTI_STUFF, device='cpu').evaluate(preds, sems, insts)
    cpu_table = capsys.readouterr().out
    for chunk in (1 << 21, 100000, 4096):
        with monkeypatch.context() as m:
            _device_only(m)
            gpu = PanopticEval(KITTI_THING, KITTI_STUFF, device='cuda', max_chunk_points=chunk).evaluate(
                preds, sems, insts)
        assert capsys.readouterr().out == cpu_table
        _pan_equal(gpu, cpu)
    # device tensors in, and evaluate_single per scan
    ev = PanopticEval(KITTI_THING, KITTI_STUFF, device='cuda')
    d = [[torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda() for x in xs]
         for xs in (preds, sems, insts)]
    d[0] = [x.to(torch.int64) & 0xFFFFFFFF for x in d[0]]
    with monkeypatch.context() as m:
        _device_only(m)
        _pan_equal(ev.evaluate(*d), cpu)
        got = ev.evaluate_single(preds[3], sems[3], insts[3])
    capsys.readouterr()
    _pan_equal(got, PanopticEval(KITTI_THING, KITTI_STUFF, device='cpu').evaluate_single(
        preds[3], sems[3], insts[3]))
    for x, y in zip(d[0], preds):
        assert np.array_equal(x.cpu().numpy(), y.astype(np.int64))


def test_semantic_large_device_equals_numpy(scannet_set):
    sp, sg, op, og, inst = scannet_set
    assert pw_mod._device_pass(sp, sg, -100, 'cuda') is not None           # no numpy fallback here
    assert pw_mod._device_pass(None, None, -100, 'cuda', inst, op, og) is not None
    a = [evaluate_semantic_miou(sp, sg, device=dv) for dv in ('cuda', 'cpu')]
    b = [evaluate_semantic_acc(sp, sg, device=dv) for dv in ('cuda', 'cpu')]
    assert a[0] == a[1] and b[0] == b[1]
    m = [evaluate_offset_mae(op, og, inst, device=dv) for dv in ('cuda', 'cuda', 'cpu')]
    assert m[0].tobytes() == m[1].tobytes()                # bitwise repeatable
    assert abs(m[0] - m[2]) <= 1e-5 * abs(m[2])
    # device tensors, int32 labels, inputs unchanged
    d = lambda xs, dt=None: [torch.from_numpy(x).cuda().to(dt or torch.from_numpy(x).dtype) for x in xs]  # noqa: E731
    sp_d, sg_d = d(sp, torch.int32), d(sg, torch.int32)
    before = [x.clone() for x in sp_d + sg_d]
    assert evaluate_semantic_miou(sp_d, sg_d) == a[1]
    assert evaluate_semantic_acc(sp_d, sg_d) == b[1]
    assert evaluate_offset_mae(d(op), d(og), d(inst)).tobytes() == m[0].tobytes()
    for x, y in zip(before, sp_d + sg_d):
        assert torch.equal(x, y)


def test_out_of_range_labels_fall_back():
    sp, sg, op, og, inst = copy.deepcopy(pc.semantic_cases()['one_scan'])
    sg[0][:5] = 5000                       # a gt class past SG_EVAL_MAX_CLASSES
    sg[0][5:9] = -7                        # and a negative one that is not the ignore value
    log_c, log_g = [], []

    class L:
        def __init__(self, out):
            self.info = out.append

    assert evaluate_semantic_miou(sp, sg, -100, L(log_g), device='cuda') == \
        evaluate_semantic_miou(sp, sg, -100, L(log_c), device='cpu')
    assert evaluate_semantic_acc(sp, sg, -100, device='cuda') == evaluate_semantic_acc(sp, sg, -100, device='cpu')
    assert log_g == log_c
    # panoptic: an instance label past int32 and a prediction past 32 bits
    thing, stuff, _, preds, sems, insts = pc.panoptic_cases()['designed']
    insts = [insts[0].copy()]
    insts[0][200:210] = 2**40
    preds = [preds[0].astype(np.int64)]
    preds[0][300:305] = 2**33 + 3
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        g = PanopticEval(thing, stuff, device='cuda').evaluate(preds, sems, insts)
        c = PanopticEval(thing, stuff, device='cpu').evaluate(preds, sems, insts)
    _pan_equal(g, c)


def test_kitti_forward_test_scored_on_device_and_numpy(capsys):
    cfg = copy.deepcopy(synthetic.KITTI_MODEL_CFG)
    model = synthetic.build_model(cfg, seed=0)
    preds, sems, insts = [], [], []
    for seed, n in ((13, 30000), (14, 22000)):
        xyz, rgb, inst = synthetic.scene_s2(seed=seed, n=n, room_scale=0.45)
        xyz = (xyz * np.float32(2.5)).astype(np.float32)
        batch = synthetic.make_batch(xyz, rgb[:, :1].copy(), scale=20, instance_labels=inst)
        with torch.no_grad():
            res = model(batch)
        preds.append(res['panoptic_preds'])
        sems.append(res['semantic_labels'])
        insts.append(res['instance_labels'])
    assert preds[0].dtype == np.uint32
    thing = [f't{i}' for i in range(cfg['instance_classes'])]
    stuff = [f's{i}' for i in range(cfg['semantic_classes'] - cfg['instance_classes'])]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        g = PanopticEval(thing, stuff, device='cuda').evaluate(preds, sems, insts)
        tg = capsys.readouterr().out
        c = PanopticEval(thing, stuff, device='cpu').evaluate(preds, sems, insts)
        tc = capsys.readouterr().out
    _pan_equal(g, c)
    assert tg == tc
