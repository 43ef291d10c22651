"""The device path of ScanNetEval(coverage=...) (sg_inst_scan_coverage, softgroup_amd/csrc/inst_eval.hip)
against the host path: integer tallies equal, doubles bit for bit -- on the shared cases, through the
grow-and-redo loop and the fallback to the host, on one scan whose labels span more GT rows than a wave and
than a workgroup, in two feeding orders, and through the C entry point on hand-built tables.  The host path
itself is checked against the dense brute force in test_coverage_eval.py (and here on the small form of the
larger scan, which needs no GPU)."""
import functools
import os
import sys

import numpy as np
import pytest

from softgroup_amd.evaluation import ScanNetEval

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'golden'))
import inst_eval_cases  # noqa: E402
from test_coverage_eval import CLASSES, PARAMS, assert_coverage_equal, brute_force  # noqa: E402

gpu = pytest.mark.gpu


def _cov(iou_thr, score_thr):
    return dict(iou_thr=iou_thr, score_thr=score_thr)


@functools.lru_cache(None)
def _cases(as_rle):
    return inst_eval_cases.cases(as_rle=as_rle)


@functools.lru_cache(None)
def _host_of_cases(as_rle, name, iou_thr, score_thr):
    pl, gl = _cases(as_rle)
    return ScanNetEval(CLASSES, device='cpu', coverage=_cov(iou_thr, score_thr),
                       **inst_eval_cases.CONFIGS[name]).evaluate(pl, gl, verbose=False)


def _device(ev, pl, gl):
    avgs = ev.evaluate(pl, gl, verbose=False, backend='device')
    assert ev.last_backend == 'device' and ev.last_fallback is None, (ev.last_backend, ev.last_fallback)
    return avgs


# ------------------------------------------------------------------------------------------ shared cases
@gpu
@pytest.mark.parametrize('iou_thr,score_thr', PARAMS)
@pytest.mark.parametrize('name', sorted(inst_eval_cases.CONFIGS))
@pytest.mark.parametrize('as_rle', [True, False])
def test_device_path_equals_the_host_path(as_rle, name, iou_thr, score_thr):
    pl, gl = _cases(as_rle)
    ev = ScanNetEval(CLASSES, coverage=_cov(iou_thr, score_thr), **inst_eval_cases.CONFIGS[name])
    assert_coverage_equal(_device(ev, pl, gl), _host_of_cases(as_rle, name, iou_thr, score_thr))
    ev.reset(backend='device')                                 # the streaming form, and reset() starts over
    for preds, gts in zip(pl, gl):
        ev.update(preds, gts)
    assert_coverage_equal(ev.compute(), _host_of_cases(as_rle, name, iou_thr, score_thr))
    assert ev.last_backend == 'device'


@gpu
@pytest.mark.parametrize('name', sorted(inst_eval_cases.CONFIGS))
def test_grow_and_redo_starts_the_accumulators_afresh(name):
    pl, gl = _cases(True)
    ev = ScanNetEval(CLASSES, coverage=True, **inst_eval_cases.CONFIGS[name])
    ev.device_capacity = dict(gt=8, examples=64)
    got = _device(ev, pl, gl)
    assert ev._dev.grown > 0
    assert_coverage_equal(got, _host_of_cases(True, name, 0.5, 0.0))


@gpu
def test_fallback_to_the_host_gives_the_host_coverage():
    pl, gl = _cases(True)
    pl, gl = pl + pl[:1], gl + gl[:1]                          # duplicate scan_id
    ev = ScanNetEval(CLASSES, coverage=True)
    got = ev.evaluate(pl, gl, verbose=False, backend='device')
    assert ev.last_backend == 'host' and 'duplicate scan_id' in ev.last_fallback
    assert_coverage_equal(got, ScanNetEval(CLASSES, device='cpu', coverage=True).evaluate(pl, gl, verbose=False))


@gpu
def test_coverage_none_on_the_device_backend_adds_no_key():
    pl, gl = _cases(True)
    ev = ScanNetEval(CLASSES)
    got = _device(ev, pl, gl)
    assert 'all_cov' not in got and 'coverage_counts' not in got and not hasattr(ev._dev, 'cov')
    assert set(got['classes'][CLASSES[0]]) == {'ap', 'ap50%', 'ap25%', 'rc', 'rc50%', 'rc25%'}


# ------------------------------------------------------------------------------------------ a larger scan
def make_scan(scan_id='big', n_points=70001, n_gt=300, n_pred=400, seed=11):
    """GT instances = consecutive blocks of 60 - 350 points (some below the minimum region size: they stay GT)
    over classes 3, 5 and 7, half of them in class 3; predictions = shifted or partial copies of a GT block,
    one in seven mislabelled (class 4 has no GT at all), exact duplicates with other confidences, and ranges
    across several GTs; confidences with ties"""
    rng = np.random.default_rng(seed)
    gts = np.zeros(n_points, np.int64)
    budget = (n_points - 200) // n_gt
    blocks, at = [], 50
    for i in range(n_gt):
        size = int(rng.integers(min(60, budget // 2), budget))
        cls = 3 if i % 2 == 0 else (5 if i % 3 else 7)
        gts[at:at + size] = cls * 1000 + i + 1
        blocks.append((at, at + size, cls))
        at += size + int(rng.integers(0, budget - size + 1))
    assert at < n_points
    preds, n_dup, n_wide = [], n_pred * 3 // 20, n_pred // 10

    def add(lo, hi, label, conf=None):
        m = np.zeros(n_points, bool)
        m[max(lo, 0):min(hi, n_points)] = True
        conf = np.float32(rng.choice([0.3, 0.5, 0.5, 0.7, round(float(rng.random()), 3)])) if conf is None else conf
        preds.append(dict(scan_id=scan_id, label_id=int(label), conf=conf, pred_mask=inst_eval_cases._rle(m)))
    for _ in range(n_pred - n_dup - n_wide):
        lo, hi, cls = blocks[int(rng.integers(0, n_gt))]
        w = hi - lo
        lo, hi = lo + int(rng.integers(-w // 3, w // 3 + 1)), hi + int(rng.integers(-w // 3, w // 3 + 1))
        add(lo, max(hi, lo + 1), cls if rng.random() < 6 / 7 else int(rng.choice([3, 4, 5, 7])))
    for _ in range(n_wide):
        lo = int(rng.integers(0, n_points - 4 * budget))
        add(lo, lo + int(rng.integers(budget, 4 * budget)), int(rng.choice([3, 5, 7])))
    for _ in range(n_dup):
        src = preds[int(rng.integers(0, len(preds)))]
        preds.append(dict(src, conf=np.float32(round(float(rng.random()), 2))))
    order = rng.permutation(len(preds))
    return [preds[i] for i in order], gts


@functools.lru_cache(None)
def _big():
    preds, gts = make_scan()
    ids = np.unique(gts[gts > 0])
    assert len(gts) == 70001 and len(preds) == 400 and len(ids) == 300
    assert sorted(set((ids // 1000).tolist())) == [3, 5, 7] and int((ids // 1000 == 3).sum()) >= 65
    return preds, gts


@functools.lru_cache(None)
def _small():
    return make_scan('small', 7001, 30, 40)


@functools.lru_cache(None)
def _host_matches(use_label, which):
    """the host path's association of one scan, made once: the evaluator, (gt2pred, pred2gt)"""
    ev = ScanNetEval(CLASSES, device='cpu', use_label=use_label, coverage=True)
    preds, gts = _big() if which == 'big' else _small()
    return ev, dict(zip(('gt', 'pred'), ev.assign_instances_for_scan(preds, gts)))


def _host_coverage(use_label, order):
    ev, _ = _host_matches(use_label, 'big')
    matches = {f'gt_{i}': _host_matches(use_label, which)[1] for i, which in enumerate(order)}
    names = ev.eval_class_labels
    return ev.add_coverage_averages({'classes': {n: {} for n in names}}, *ev.coverage_of_matches(matches))


def test_host_path_on_the_small_form_of_the_larger_scan_equals_the_brute_force():
    preds, gts = _small()
    for use_label in (True, False):
        want = brute_force([preds], [gts], CLASSES, use_label=use_label)
        assert int(want['coverage_counts']['tp'].sum()) > 0 and int(want['coverage_counts']['fp'].sum()) > 0
        got = ScanNetEval(CLASSES, device='cpu', use_label=use_label, coverage=True).evaluate(
            [preds], [gts], verbose=False)
        assert_coverage_equal(got, want)


@gpu
@pytest.mark.parametrize('use_label', [True, False])
def test_larger_scan_equals_the_host_path(use_label):
    preds, gts = _big()
    ev = ScanNetEval(CLASSES, use_label=use_label, coverage=True)
    if not use_label:
        ev.device_capacity = dict(gt=512)                      # one label of 300 GT rows, tables large enough at once
    got = _device(ev, [preds], [gts])
    assert ev._dev.grown == (1 if use_label else 0)            # (the default tables hold 256 GT rows)
    want = _host_coverage(use_label, ['big'])
    assert int(want['coverage_counts']['n_gt'].sum()) == 300
    assert min(int(want['coverage_counts'][k].sum()) for k in ('tp', 'fp', 'gt_hit')) > 20     # not hollow
    assert_coverage_equal(got, want)


@gpu
def test_feeding_order_decides_the_sums_as_on_the_host():
    preds, gts = _big()
    other_p, other_g = _small()
    again = [dict(p, scan_id='big2') for p in preds]
    feeds = {('big', 'big', 'other'): [(preds, gts), (again, gts), (other_p, other_g)],
             ('other', 'big', 'big'): [(other_p, other_g), (again, gts), (preds, gts)]}
    got = {}
    for order, scans in feeds.items():
        ev = ScanNetEval(CLASSES, coverage=True, backend='device')
        ev.device_capacity = dict(gt=512)
        ev.reset()
        for p, g in scans:
            ev.update(p, g)
        got[order] = ev.compute()
        assert ev.last_backend == 'device' and ev._dev.grown == 0
        assert_coverage_equal(got[order], _host_coverage(True, order))
    a, b = (_host_coverage(True, o) for o in feeds)
    assert all(np.array_equal(a['coverage_counts'][k], b['coverage_counts'][k]) for k in a['coverage_counts'])


# ------------------------------------------------------------------------------------------ the entry point
def _raw(gts, preds, iou_thr=0.5, score_thr=0.0, times=1, n_classes=3, min_region=10, gt_cap=8):
    """sg_inst_scan_update + sg_inst_scan_coverage through ctypes, `times` times over the same accumulators.
    preds: (lo, hi, label index, conf).  -> (sums [2][n_classes], tallies [5][n_classes])"""
    import torch
    from softgroup_amd import _lib as L
    lib, n, n_pred = L.lib(), len(gts), len(preds)
    dev = torch.device('cuda')

    def d(a, dtype):
        return torch.from_numpy(np.asarray(a, dtype).reshape(-1)).to(dev) if len(a) else None
    d_gts = d(gts, np.int64)
    start, length = d([p[0] for p in preds], np.int32), d([p[1] - p[0] for p in preds], np.int32)
    owner, label = d(list(range(n_pred)), np.int32), d([p[2] for p in preds], np.int32)
    vert, conf = d([p[1] - p[0] for p in preds], np.int32), d([p[3] for p in preds], np.float64)
    thr = np.array([0.5], np.float64)
    ex_key, ex_meta = torch.zeros(64, dtype=torch.int64, device=dev), torch.zeros(64, dtype=torch.int32, device=dev)
    seg_stats = torch.zeros(4 * n_classes, dtype=torch.int32, device=dev)
    meta = torch.zeros(4, dtype=torch.int64, device=dev)
    cov = torch.zeros(7 * n_classes, dtype=torch.int64, device=dev)
    size = (n, n_pred, n_pred, n_classes, gt_cap, 1, n_classes)
    ws_bytes = lib.sg_inst_scan_workspace_bytes(*size, None)
    assert ws_bytes > 0
    ws = L.workspace(ws_bytes, dev)
    flags = meta.data_ptr() + 16
    for _ in range(times):
        L.check(lib.sg_inst_scan_update(L.ptr(d_gts), n, L.ptr(start), L.ptr(length), L.ptr(owner), n_pred,
                                        L.ptr(label), L.ptr(vert), L.ptr(conf), n_pred, n_classes, n_classes,
                                        min_region, thr.ctypes.data, 1, gt_cap, ex_key.data_ptr(), ex_meta.data_ptr(),
                                        64, seg_stats.data_ptr(), meta.data_ptr(), flags, ws.data_ptr(), ws_bytes,
                                        L.stream()), 'sg_inst_scan_update')
        L.check(lib.sg_inst_scan_coverage(*size, L.ptr(label), L.ptr(vert), L.ptr(conf), min_region, iou_thr,
                                          score_thr, cov.data_ptr(), cov.data_ptr() + 16 * n_classes, flags,
                                          ws.data_ptr(), ws_bytes, L.stream()), 'sg_inst_scan_coverage')
    out = cov.cpu().numpy()
    assert int(meta.cpu()[2]) == 0
    return out[:2 * n_classes].view(np.float64).reshape(2, n_classes), out[2 * n_classes:].reshape(5, n_classes)


def _hand_gts():
    gts = np.zeros(1000, np.int64)
    gts[0:100], gts[100:300], gts[400:500] = 1001, 1002, 2001
    return gts


@gpu
def test_entry_point_on_hand_built_tables():
    # label 0: one GT half covered (IoU exactly 0.5), one GT without any overlapping prediction (ov 0 counts in
    # the means); label 1: a GT and no prediction; label 2: a prediction and no GT (an fp, no room)
    preds = [(0, 50, 0, 0.9), (600, 700, 2, 0.8), (800, 805, 0, 0.9)]      # the last one is below min_region
    cov0, wcov0 = (0.5 + 0.0) / 2.0, (0.5 * 100.0 + 0.0 * 200.0) / 300.0
    sums, t = _raw(_hand_gts(), preds)
    assert t.tolist() == [[1, 1, 0], [2, 1, 0], [1, 0, 0], [1, 0, 0], [0, 0, 1]]
    assert sums.tolist() == [[cov0, 0.0, 0.0], [wcov0, 0.0, 0.0]]
    # >= at the threshold, > above it
    _, t = _raw(_hand_gts(), preds, iou_thr=float(np.nextafter(0.5, 1.0)))
    assert t[2].tolist() == [0, 0, 0] and t[3].tolist() == [0, 0, 0] and t[4].tolist() == [1, 0, 1]
    # a score threshold removes the prediction from both sides
    sums, t = _raw(_hand_gts(), preds, score_thr=0.85)
    assert t.tolist() == [[1, 1, 0], [2, 1, 0], [1, 0, 0], [1, 0, 0], [0, 0, 0]]
    sums, t = _raw(_hand_gts(), preds, score_thr=0.95)
    assert t.tolist() == [[1, 1, 0], [2, 1, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]] and not sums.any()


@gpu
def test_entry_point_accumulates_over_calls():
    preds = [(0, 50, 0, 0.9), (600, 700, 2, 0.8)]
    cov0, wcov0 = (0.5 + 0.0) / 2.0, (0.5 * 100.0 + 0.0 * 200.0) / 300.0
    sums, t = _raw(_hand_gts(), preds, times=3)
    assert t.tolist() == [[3, 3, 0], [6, 3, 0], [3, 0, 0], [3, 0, 0], [0, 0, 3]]
    assert sums.tolist() == [[cov0 + cov0 + cov0, 0.0, 0.0], [wcov0 + wcov0 + wcov0, 0.0, 0.0]]


@gpu
def test_entry_point_without_predictions_without_gt_and_on_an_empty_scan():
    sums, t = _raw(_hand_gts(), [])
    assert t.tolist() == [[1, 1, 0], [2, 1, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]] and not sums.any()
    sums, t = _raw(np.zeros(1000, np.int64), [(0, 50, 0, 0.9), (600, 700, 2, 0.8)])
    assert t.tolist() == [[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [1, 0, 1]] and not sums.any()
    sums, t = _raw(np.zeros(0, np.int64), [])
    assert not t.any() and not sums.any()


def test_entry_point_rejects_bad_arguments_without_a_launch():
    from softgroup_amd import _lib as L
    lib = L.lib()
    assert lib.sg_inst_scan_coverage(1000, 0, 0, 3, 8, 1, 3, None, None, None, 10, 0.5, 0.0, None, None, None,
                                     None, 0, None) < 0
    assert b'sg_inst_scan_coverage' in lib.sg_last_error()
    assert lib.sg_inst_scan_coverage(1000, 0, 0, 3, 8, 1, 3, None, None, None, 10, float('nan'), 0.0, 1, 1, 1,
                                     1, 1 << 20, None) < 0
