"""Box detection AP on the GPU (sg_det_boxes_runs, sg_det_boxes_labels, sg_det_match): against the
reference's outputs in box_eval_golden.json, against the numpy path bit for bit on large random sets
with heavy confidence ties, box extraction at ScanNet size (float32 / float64, RLE / dense, negative
coordinates, many scans per launch), the non-finite fallback, one multi-threshold pass against single
calls, end to end from a synthetic forward_test, and tools/eval_det.py device against cpu."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from softgroup_amd import synthetic
from softgroup_amd.evaluation import det_eval as de
from softgroup_amd.evaluation import eval_sphere, evaluate_box_ap
from softgroup_amd.util.rle import rle_encode

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'golden'))
import box_eval_cases as bc  # noqa: E402
from test_box_eval import GOLD, check_cls, check_det, check_scene, same  # noqa: E402

pytestmark = pytest.mark.gpu


def _device_only(monkeypatch):
    """make a host fallback an error: the device path must carry these inputs"""
    def boom(*a, **k):
        raise AssertionError('host path taken')
    for name in ('_match_numpy', '_match_reference_loop', '_boxes_numpy'):
        monkeypatch.setattr(de, name, boom)


def _res_equal(a, b):
    ra, pa, aa = a
    rb, pb, ab = b
    assert list(aa) == list(ab)
    for k in aa:
        assert same(ra[k], rb[k]) and same(pa[k], pb[k]) and same(aa[k], ab[k]), k


@pytest.mark.parametrize('name', sorted(GOLD['det']))
def test_eval_det_device_equals_reference(name, monkeypatch):
    _device_only(monkeypatch)
    check_det(name, 'cuda')


def test_eval_det_cls_device_equals_reference(monkeypatch):
    _device_only(monkeypatch)
    check_cls('cuda')


@pytest.mark.parametrize('name', sorted(GOLD['scenes']))
def test_evaluate_box_ap_device_equals_reference(name, monkeypatch):
    _device_only(monkeypatch)
    check_scene(name, 'cuda')


def _tied_set(seed, n_img=40, n_det=60):
    pred_all, gt_all = bc.random_case(seed, n_img=n_img, n_cls=5, n_gt=25, n_det=n_det, jitter=0.25)
    rng = np.random.default_rng(seed + 1)
    # heavy ties: 21 distinct %.4f scores
    pred_all = {img: [(c, b, float(f'{rng.integers(0, 21) / 20:.4f}')) for c, b, _ in p] for img, p in pred_all.items()}
    return pred_all, gt_all


@pytest.mark.parametrize('seed', [11, 12])
def test_device_equals_numpy_with_heavy_ties(seed):
    pred_all, gt_all = _tied_set(seed)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        for t in bc.THRESHOLDS:
            for u07 in (False, True):
                _res_equal(eval_sphere(pred_all, gt_all, t, u07, device='cuda'),
                           eval_sphere(pred_all, gt_all, t, u07, device='cpu'))


def test_match_kernel_ovmax_jmax_equal_numpy():
    pred_all, gt_all = _tied_set(13, n_img=30)
    pred, gt = de._by_class(pred_all, gt_all)
    jobs = [de._ClassJob(pred[c], gt[c]) for c in gt if c in pred]
    det_box, det_group, det_rank, gt_box, sizes, want_ov, want_j = [], [], [], [], [], [], []
    for job in jobs:
        base = len(sizes)
        g0 = sum(sizes)
        imgs = list(job.gt_sphere)
        for img in imgs:
            s = job.gt_sphere[img]
            sizes.append(len(s) if s.size else 0)
            if s.size:
                gt_box.append(s.reshape(-1, 6))
        det_box.append(job.BB.reshape(-1, 6))
        det_group.append(np.array([base + imgs.index(i) for i in job.image_ids], np.int32))
        rank = np.empty(job.nd, np.int32)
        rank[job.sorted_ind] = np.arange(job.nd)
        det_rank.append(rank)
        goff = np.concatenate([[0], np.cumsum(sizes[base:])])
        for d in range(job.nd):
            G = job.gt_sphere[job.image_ids[d]]
            iou = de._iou_rows(job.BB[d].astype(float), G.reshape(-1, 6).astype(float)) if G.size else np.zeros(0)
            if len(iou):
                j = int(np.argmax(iou))
                want_ov.append(iou[j])
                want_j.append(g0 + goff[imgs.index(job.image_ids[d])] + j)
            else:
                want_ov.append(-np.inf)
                want_j.append(-1)
    ov, jm, tp = de.match_boxes(np.concatenate(det_box), np.concatenate(det_group), np.concatenate(det_rank),
                                np.concatenate(gt_box), np.array(sizes), bc.THRESHOLDS, torch.device('cuda'))
    assert same(ov, want_ov) and np.array_equal(jm, want_j)
    assert tp.shape == (2, len(ov)) and tp.any()


def test_multi_threshold_pass_equals_single_calls():
    pred_all, gt_all = _tied_set(14)
    ths = [0.1, 0.25, 0.5, 0.7]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        multi = de._eval_multi(pred_all, gt_all, ths, False, de.get_iou, 'cuda', 'zero')
        for t, res in zip(ths, multi):
            _res_equal(res, eval_sphere(pred_all, gt_all, t, device='cuda'))


def _scans(dtype, n_scans, n, seed, negative=False):
    rng = np.random.default_rng(seed)
    coords, masks, insts = [], [], []
    for s in range(n_scans):
        xyz = rng.uniform(-4 if negative else 0, 4, (n, 3)).astype(dtype)
        k = 40
        inst = rng.integers(0, k, n)
        inst = np.sort(inst)[np.argsort(rng.uniform(size=n) < 0.7, kind='stable')]   # runs + scatter
        inst[rng.uniform(size=n) < 0.1] = -100
        inst[:k] = np.arange(k)
        ms = []
        for p in range(100):
            m = inst == rng.integers(0, k)
            m ^= rng.uniform(size=n) < 0.002
            m[rng.integers(0, n)] = True
            ms.append(m)
        coords.append(xyz)
        masks.append(ms)
        insts.append(inst.astype(np.int64))
    return coords, masks, insts


def _boxes_equal(a, b):
    (pa, ga), (pb, gb) = a, b
    assert len(pa) == len(pb) and len(ga) == len(gb)
    for x, y in zip(pa, pb):
        assert x.shape == y.shape and same(x, y)                  # == : +-0.0 may differ in sign only
    for (bx, cx, fx), (by, cy, fy) in zip(ga, gb):
        assert same(bx, by) and np.array_equal(cx, cy) and np.array_equal(fx, fy)


@pytest.mark.parametrize('dtype,rle,negative,n_scans,n', [
    (np.float32, False, False, 2, 150000), (np.float64, True, True, 2, 150000),
    (np.float32, True, True, 12, 6000), (np.float64, False, False, 1, 150000)])
def test_box_extraction_equals_numpy(dtype, rle, negative, n_scans, n, monkeypatch):
    coords, masks, insts = _scans(dtype, n_scans, n, seed=n_scans, negative=negative)
    if rle:
        masks = [[rle_encode(m.astype(np.int64)) for m in ms] for ms in masks]
    want = de.instance_boxes(coords, masks, insts, device='cpu')
    _device_only(monkeypatch)
    got = de.instance_boxes(coords, masks, insts, device='cuda')
    _boxes_equal(got, want)
    assert all(np.isfinite(p).all() for p in got[0])


def test_non_finite_coordinate_takes_host_path():
    coords, masks, insts = _scans(np.float32, 2, 5000, seed=5)
    coords = [c.copy() for c in coords]
    p = int(np.flatnonzero(masks[1][3])[0])
    coords[1][p, 1] = np.nan
    coords[0][int(np.flatnonzero(insts[0] == 7)[0]), 2] = np.inf
    runs = [[tuple(np.asarray(x, np.int64) for x in de._runs_of(m, len(c))) for m in ms]
            for c, ms in zip(coords, masks)]
    assert de._boxes_device(coords, runs, insts, 'cuda') is None     # the kernel flags it
    got = de.instance_boxes(coords, masks, insts, device='cuda')
    want = de.instance_boxes(coords, masks, insts, device='cpu')
    _boxes_equal(got, want)
    assert np.isnan(got[0][1][3, 1]) and np.isinf(got[1][0][0][7, 5])


def test_forward_test_scored_on_device_and_numpy():
    model = synthetic.build_model(seed=0)
    preds, coords, sems, insts = [], [], [], []
    for seed, n in ((21, 30000), (22, 24000)):
        xyz, rgb, inst = synthetic.scene_s2(seed=seed, n=n, room_scale=0.45)
        batch = synthetic.make_batch(xyz, rgb, instance_labels=inst)
        with torch.no_grad():
            res = model(batch)
        preds.append(res['pred_instances'])
        coords.append(res['coords_float'])
        sems.append(res['semantic_labels'])
        insts.append(res['instance_labels'])
    assert sum(len(p) for p in preds) > 0
    names = [f'c{i}' for i in range(18)]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        g = evaluate_box_ap(preds, coords, sems, insts, names, device='cuda')
        c = evaluate_box_ap(preds, coords, sems, insts, names, device='cpu')
    for t in bc.THRESHOLDS:
        _res_equal((g[t]['rec'], g[t]['prec'], g[t]['ap']), (c[t]['rec'], c[t]['prec'], c[t]['ap']))
        assert same(g[t]['mAP'], c[t]['mAP'])


def test_eval_det_tool_device_equals_cpu(tmp_path):
    data, results = bc.write_out_tree(str(tmp_path), 'f64_negative')
    outs = []
    for device in ('cuda', 'cpu'):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'eval_det.py'), '--data-path', data,
                            '--results-path', results, '--iou', '0.25', '0.5', '--device', device],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs.append([ln for ln in r.stdout.splitlines() if ln.startswith(('mAP', 'IoU'))])
    assert outs[0] == outs[1] and len(outs[0]) == 4
    g = GOLD['scenes']['f64_negative']
    assert outs[0][1] == f"mAP: {g['0.25']['mAP']}" and outs[0][3] == f"mAP: {g['0.5']['mAP']}"
