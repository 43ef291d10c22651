"""The device path of ScanNetEval (softgroup_amd/csrc/inst_eval.hip): values against the reference's
golden averages and the host backend, the stages against numpy, the shapes that cross the kernels'
internal boundaries, and the fallbacks.  Every value test asserts that the device path really ran."""
import functools
import json
import math
import os
import sys

import numpy as np
import pytest

from softgroup_amd.evaluation import ScanNetEval
from softgroup_amd.evaluation.instance_eval import _runs_of

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import eval_cases  # noqa: E402
import inst_eval_cases  # noqa: E402

GOLD = json.load(open(os.path.join(HERE, 'golden', 'inst_eval_golden.json')))
GOLD_OLD = json.load(open(os.path.join(HERE, 'golden', 'eval_golden.json')))
CLASSES = list(inst_eval_cases.CLASSES)


def _same(a, b, key=''):
    """rc figures exactly, ap figures to 1e-12: fewer than 4 096 unique thresholds per case, so a reordered
    sum of terms in [0, 1] differs by at most 4096 * 2**-52 ~ 9e-13; NaN equals NaN"""
    if isinstance(b, dict):
        assert set(a) == set(b)
        for k in b:
            _same(a[k], b[k], k)
    else:
        a, b = float(a), float(b)
        if math.isnan(a) and math.isnan(b):
            return
        print(key, a, b, abs(a - b))
        if 'rc' in key:
            assert a == b, (key, a, b)
        else:
            assert abs(a - b) <= 1e-12, (key, a, b)


def _device(ev, pl, gl):
    avgs = ev.evaluate(pl, gl, verbose=False, backend='device')
    assert ev.last_backend == 'device' and ev.last_fallback is None, (ev.last_backend, ev.last_fallback)
    return avgs


def _host(pl, gl, **kw):
    return ScanNetEval(CLASSES, device='cpu', **kw).evaluate(pl, gl, verbose=False)


# ------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize('name', sorted(inst_eval_cases.CONFIGS))
@pytest.mark.parametrize('as_rle', [True, False])
def test_device_backend_equals_the_reference(name, as_rle):
    pl, gl = inst_eval_cases.cases(as_rle=as_rle)
    ev = ScanNetEval(CLASSES, **inst_eval_cases.CONFIGS[name])
    _same(_device(ev, pl, gl), GOLD[name])


def test_streaming_form_device_tensors_and_repeatability():
    import torch
    pl, gl = inst_eval_cases.cases()
    ev = ScanNetEval(CLASSES, backend='device')
    runs = []
    for as_tensor in (False, True):
        ev.reset()
        for preds, gts in zip(pl, gl):
            ev.update(preds, torch.from_numpy(gts).cuda().to(torch.int32) if as_tensor else gts)
        runs.append(ev.compute())
        assert ev.last_backend == 'device' and ev.last_fallback is None
    _same(runs[0], GOLD['class_aware'])
    assert json.dumps(runs[0], default=lambda x: float(x).hex(), sort_keys=True) == \
        json.dumps(runs[1], default=lambda x: float(x).hex(), sort_keys=True)      # bit-identical


@pytest.mark.parametrize('name', sorted(inst_eval_cases.CONFIGS))
def test_existing_cases_through_the_device_backend(name):
    pl, gl = eval_cases.cases()
    _same(_device(ScanNetEval(CLASSES, **inst_eval_cases.CONFIGS[name]), pl, gl), GOLD_OLD[name])


def test_model_forward_evaluated_by_both_backends():
    import torch
    from softgroup_amd import synthetic
    xyz, rgb, inst = synthetic.scene_s2(seed=3, n=30000, room_scale=0.45)
    model = synthetic.build_model(seed=0)
    with torch.no_grad():
        out = model(synthetic.make_batch(xyz, rgb, instance_labels=inst))
    ev = ScanNetEval(CLASSES)
    a = _device(ev, [out['pred_instances']], [out['gt_instances']])
    b = ev.evaluate([out['pred_instances']], [out['gt_instances']], verbose=False)
    assert ev.last_backend == 'host'
    _same(a, b)


# ------------------------------------------------------------------------------------------ stages
def test_rle_text_parse_against_runs_of():
    import torch
    from softgroup_amd import _lib as L
    n = 5000
    rng = np.random.default_rng(0)
    masks = [np.zeros(n, bool), np.zeros(n, bool), np.arange(n) % 2 == 0, rng.random(n) < 0.5, np.ones(n, bool),
             np.zeros(n, bool)]
    masks[1][17:4000] = True                               # a single run
    masks[5][n - 1] = True                                 # the last point; its text ends the buffer
    rles = [inst_eval_cases._rle(m) for m in masks] + [dict(length=n, counts='')]    # an empty mask at the end
    texts = [r['counts'] for r in rles]
    assert len(texts[2].split()) // 2 > 1024
    text = ''.join(texts).encode()
    off = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64)
    lib = L.lib()
    slots = lib.sg_inst_rle_run_slots(len(text), len(texts))
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()      # exactly len(text) bytes
    d_off = torch.from_numpy(off).cuda()
    runs = torch.full((3, slots), -7, dtype=torch.int32, device='cuda')
    vert = torch.full((len(texts),), -7, dtype=torch.int32, device='cuda')
    flags = torch.zeros(1, dtype=torch.int32, device='cuda')
    L.check(lib.sg_inst_rle_parse(d_text.data_ptr(), d_off.data_ptr(), None, len(texts), len(text), n,
                                  runs[0].data_ptr(), runs[1].data_ptr(), runs[2].data_ptr(), slots,
                                  vert.data_ptr(), flags.data_ptr(), L.stream()), 'parse')
    r, v = runs.cpu().numpy(), vert.cpu().numpy()
    assert int(flags.cpu()) == 0
    used = np.zeros(slots, bool)
    for m, rle in enumerate(rles):
        s, ln = _runs_of(rle, n)
        b = (off[m] + m) // 4
        assert np.array_equal(r[0, b:b + len(s)], s) and np.array_equal(r[1, b:b + len(s)], ln)
        assert (r[2, b:b + len(s)] == m).all() and v[m] == ln.sum()
        used[b:b + len(s)] = True
    assert (r[1][~used] == 0).all() and (r[0][~used] == 0).all()       # spare slots are empty runs
    assert r[1].sum() == sum(int(m.sum()) for m in masks)


def _tables(ev, preds, gts, gt_cap=64):
    """the scan's tables as sg_inst_scan_update left them in its workspace"""
    import ctypes
    from softgroup_amd import _lib as L
    ev.device_capacity = dict(gt=gt_cap)
    ev.reset(backend='device')
    ev.update(preds, gts)
    acc = ev._dev
    last = acc._last
    off = (ctypes.c_int64 * 16)()
    nb = L.lib().sg_inst_scan_workspace_bytes(last['n_points'], last['n_pred'], last['run_slots'], acc.n_classes,
                                              acc.gt_cap, acc.n_thr, acc.n_labels, off)
    assert nb == last['ws'].numel() or nb <= 256
    raw = last['ws'].cpu().numpy()
    n_pred = last['n_pred']

    def sec(i, dtype, count):
        return raw[off[i]:off[i] + count * np.dtype(dtype).itemsize].view(dtype)
    n_gt, _, n_pairs = sec(0, np.int32, 3)
    t = dict(n_gt=int(n_gt), n_pairs=int(n_pairs), vert=last['vert'].cpu().numpy())
    for i, k in ((1, 'gt_id'), (2, 'gt_label'), (3, 'gt_vert')):
        t[k] = sec(i, np.int32, n_gt)
    t['pred_void'] = sec(6, np.int32, n_pred)
    t['by_gt'] = [sec(i, np.float64 if i == 10 else np.int32, n_pairs) for i in (7, 8, 9, 10)]
    t['by_pred'] = [sec(i, np.float64 if i == 14 else np.int32, n_pairs) for i in (11, 12, 13, 14)]
    assert ev._dev.fallback is None
    return t


@pytest.mark.parametrize('use_label', [True, False])
def test_gt_table_and_pair_records_against_the_host_association(use_label):
    pl, gl = inst_eval_cases.cases()
    for scan in (0, 3):
        preds, gts = pl[scan], gl[scan]
        ev = ScanNetEval(CLASSES, use_label=use_label)
        t = _tables(ev, preds, gts)
        # GT table = np.unique's ids of evaluated classes, ascending, with their point counts
        ids, cnt = np.unique(gts, return_counts=True)
        keep = (ids != 0) & np.isin(ids // 1000, ev.valid_class_ids)
        assert np.array_equal(t['gt_id'], ids[keep]) and np.array_equal(t['gt_vert'], cnt[keep])
        assert np.array_equal(t['gt_label'], ids[keep] // 1000 - 1 if use_label else np.zeros(keep.sum()))
        # pair records in the host's two orders
        host = ScanNetEval(CLASSES, use_label=use_label, device='cpu')
        gt2pred, pred2gt = host.assign_instances_for_scan(preds, gts)
        verts = [int(_runs_of(p['pred_mask'], len(gts))[1].sum()) for p in preds]
        kept = [i for i, p in enumerate(preds) if (not use_label or p['label_id'] in host.id2label) and verts[i] >= 100]
        assert all(t['vert'][i] == verts[i] for i in kept)
        all_gt = sorted((g for lst in gt2pred.values() for g in lst), key=lambda g: g['instance_id'])
        by_gt = [(g['instance_id'], kept[p['pred_id']], p['intersection'], p['iou'])
                 for g in all_gt for p in g['matched_pred']]
        all_pred = sorted((p for lst in pred2gt.values() for p in lst), key=lambda p: p['pred_id'])
        by_pred = [(g['instance_id'], kept[p['pred_id']], g['intersection'], g['iou'])
                   for p in all_pred for g in p['matched_gt']]
        assert len(by_gt) == t['n_pairs'] > 0
        for want, (g, p, inter, iou) in ((by_gt, t['by_gt']), (by_pred, t['by_pred'])):
            got = list(zip(t['gt_id'][g].tolist(), p.tolist(), inter.tolist(), iou.tolist()))
            assert got == want                              # IoUs bit for bit
        for p in all_pred:
            assert t['pred_void'][kept[p['pred_id']]] == p['void_intersection']


# ------------------------------------------------------------------------------------------ boundaries
def _blocks(scan, n, items, seed):
    """items: (lo, hi, label); confidences with ties"""
    rng = np.random.default_rng(seed)
    preds = []
    for lo, hi, label in items:
        m = np.zeros(n, bool)
        m[lo:hi] = True
        preds.append(dict(scan_id=scan, label_id=label, conf=np.float32(round(float(rng.random()), 2)),
                          pred_mask=inst_eval_cases._rle(m)))
    return preds


@functools.lru_cache(None)
def _wave_case():
    n = 3000
    gts = np.zeros(n, np.int64)
    gts[0:1000], gts[1000:1500], gts[1500:2000] = 3001, 3002, 5003
    a = _blocks('w0', n, [(0, 1000 - 3 * i, 3) for i in range(70)], 1)          # 70 predictions on one GT
    b = _blocks('w1', n, [(1000 + 5 * i, 1500, 3) if i % 2 else (1500, 2000 - 4 * i, 5) for i in range(65)], 2)
    return [a, b], [gts, gts.copy()]


def test_more_predictions_than_a_wave():
    pl, gl = _wave_case()
    assert len(pl[0]) == 70 and len(pl[1]) == 65
    _same(_device(ScanNetEval(CLASSES), pl, gl), _host(pl, gl))


@functools.lru_cache(None)
def _long_segment_case():
    n = 24000
    pl, gl = [], []
    for s in range(9):
        gts = np.zeros(n, np.int64)
        for g in range(24):
            gts[1000 * g:1000 * (g + 1)] = 3001 + g
        items = [(1000 * i, 1000 * (i + 1), 3) for i in range(3)]               # three true positives
        items += [(100 * i, 100 * (i + 1), 3) for i in range(30, 240)]          # IoU 0.1: false positives
        items += [(100 * i, 100 * i + 150, 3) for i in range(0, 27)]
        pl.append(_blocks(f'long{s}', n, items, 10 + s))
        gl.append(gts)
    return pl, gl, _host(pl, gl)


def test_segment_longer_than_the_sort_and_scan_tiles():
    pl, gl, want = _long_segment_case()
    assert sum(len(p) for p in pl) == 9 * 240 >= 2049
    ev = ScanNetEval(CLASSES)
    _same(_device(ev, pl, gl), want)
    assert int(ev._dev.seg_stats[:ev._dev.n_seg].max()) >= 2049               # one (label, threshold) segment


def test_no_predictions_and_no_gt_at_all():
    pl, gl = inst_eval_cases.cases()
    with np.errstate(all='ignore'):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            none = [[] for _ in pl]
            _same(_device(ScanNetEval(CLASSES), none, gl), _host(none, gl))
            empty = [np.zeros_like(g) for g in gl]
            _same(_device(ScanNetEval(CLASSES), pl, empty), _host(pl, empty))
            _same(_device(ScanNetEval(CLASSES), [], []), _host([], []))


# ------------------------------------------------------------------------------------------ fallbacks
def _fallback(pl, gl, reason, **kw):
    ev = ScanNetEval(CLASSES, **kw)
    got = ev.evaluate(pl, gl, verbose=False, backend='device')
    assert ev.last_backend == 'host' and reason in ev.last_fallback, ev.last_fallback
    _same(got, _host(pl, gl, **kw))


def test_fallbacks_give_the_host_result_and_the_reason():
    pl, gl = inst_eval_cases.cases()
    _fallback(pl + pl[:1], gl + gl[:1], 'duplicate scan_id')
    big = [g.copy() for g in gl]
    big[3][:50] = 3_000_000_000
    _fallback(pl, big, '2**31')
    neg = [g.copy() for g in gl]
    neg[0][3990:] = -5
    _fallback(pl, neg, 'negative')
    nan = [list(p) for p in pl]
    nan[0][10] = dict(nan[0][10], conf=float('nan'))
    _fallback(nan, gl, 'non-finite')


def test_reference_indexerror_case_is_handed_to_the_host():
    """a label whose only GT stays unmatched and whose only prediction is ignored (it lies on unannotated
    points): GT and predictions but no example, where the reference indexes an empty array"""
    gts = np.zeros(3000, np.int64)
    gts[:200] = 3001
    pl, gl = [_blocks('ie', 3000, [(1000, 1300, 3)], 0)], [gts]
    with pytest.raises(IndexError):
        _host(pl, gl)
    ev = ScanNetEval(CLASSES)
    with pytest.raises(IndexError):
        ev.evaluate(pl, gl, verbose=False, backend='device')
    assert ev.last_backend == 'host' and 'IndexError' in ev.last_fallback


def test_tiny_capacity_grows():
    pl, gl = inst_eval_cases.cases()
    ev = ScanNetEval(CLASSES)
    ev.device_capacity = dict(examples=8, gt=2)
    got = ev.evaluate(pl, gl, verbose=False, backend='device')
    _same(got, GOLD['class_aware'])
    if ev.last_backend == 'device':
        assert ev.last_fallback is None and ev._dev.grown >= 1
    else:
        assert 'capacity' in ev.last_fallback


@pytest.mark.parametrize('counts', ['1 5 x 3', '1 5 9', '1 5 3999 3', '1 5 -2 3', '1 99999999999999'])
def test_malformed_rle_text_raises(counts):
    pl, gl = inst_eval_cases.cases()
    bad = [list(p) for p in pl]
    bad[0][0] = dict(bad[0][0], pred_mask=dict(length=len(gl[0]), counts=counts))
    with pytest.raises(ValueError, match='malformed RLE'):
        ScanNetEval(CLASSES).evaluate(bad, gl, verbose=False, backend='device')
