"""ScanNetEval(coverage=...): mean coverage, size-weighted coverage, precision and recall (the S3DIS
columns) on the host backend against a brute force over dense masks that restates the definitions of
softgroup_amd/evaluation/instance_eval.py word for word.  Integer tallies must be equal, doubles bit-equal,
NaNs in the same places.  The device path is checked against the host path in test_coverage_eval_gpu.py."""
import math
import os
import sys

import numpy as np
import pytest

from softgroup_amd.evaluation import ScanNetEval
from softgroup_amd.util.rle import rle_decode

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import inst_eval_cases  # noqa: E402

CLASSES = list(inst_eval_cases.CLASSES)
TALLIES = ('rooms', 'n_gt', 'gt_hit', 'tp', 'fp')
KEYS = ('cov', 'wcov', 'prec', 'rec')
PARAMS = [(0.5, 0.0), (0.25, 0.0), (0.5, 0.5), (0.25, 0.5)]
NAN = float('nan')


# ------------------------------------------------------------------------------------------ brute force
def _dense(mask):
    return rle_decode(mask).astype(bool) if isinstance(mask, dict) else np.asarray(mask) != 0


def brute_force(pred_list, gt_list, classes, use_label=True, min_npoint=None, iou_thr=0.5, score_thr=0.0,
                detail=None):
    """the definitions on dense bool masks: a double loop over GT x predictions per label.  -> the keys the
    evaluator adds to avgs.  detail (a list) receives every ov_pred."""
    n_cls = len(classes)
    names = list(classes) if use_label else ['class_agnostic']
    min_region = min_npoint if min_npoint else 100
    cov_sum, wcov_sum = [0.0] * len(names), [0.0] * len(names)
    cnt = {k: [0] * len(names) for k in TALLIES}
    for preds, gts in zip(pred_list, gt_list):
        gts = np.asarray(gts)
        gt_ids = [int(i) for i in np.unique(gts) if 1 <= int(i) // 1000 <= n_cls]      # ascending, all sizes
        gt_mask = {i: gts == i for i in gt_ids}
        part = []                                              # participating predictions: (label index, mask)
        for p in preds:
            if use_label and not 1 <= p['label_id'] <= n_cls:
                continue
            m = _dense(p['pred_mask'])
            if int(m.sum()) >= min_region and float(p['conf']) >= score_thr:
                part.append((p['label_id'] - 1 if use_label else 0, m))
        for li in range(len(names)):
            G = [i for i in gt_ids if not use_label or i // 1000 - 1 == li]
            P = [m for lab, m in part if lab == li]

            def iou(g, m):
                inter = int(np.logical_and(gt_mask[g], m).sum())
                return inter / (int(gt_mask[g].sum()) + int(m.sum()) - inter)
            if G:
                s = w = 0.0
                vert = 0
                for g in G:
                    ov = max([iou(g, m) for m in P], default=0.0)
                    s = s + ov
                    w = w + ov * float(gt_mask[g].sum())
                    vert += int(gt_mask[g].sum())
                    cnt['gt_hit'][li] += ov >= iou_thr
                cnt['rooms'][li] += 1
                cnt['n_gt'][li] += len(G)
                cov_sum[li] = cov_sum[li] + s / len(G)
                wcov_sum[li] = wcov_sum[li] + w / vert
            for m in P:
                ov = max([iou(g, m) for g in G], default=0.0)
                cnt['tp' if ov >= iou_thr else 'fp'][li] += 1
                if detail is not None:
                    detail.append(ov)

    def div(a, b):
        return a / b if b else NAN
    cols = dict(cov=[div(cov_sum[li], cnt['rooms'][li]) for li in range(len(names))],
                wcov=[div(wcov_sum[li], cnt['rooms'][li]) for li in range(len(names))],
                prec=[div(cnt['tp'][li], cnt['tp'][li] + cnt['fp'][li]) for li in range(len(names))],
                rec=[div(cnt['gt_hit'][li], cnt['n_gt'][li]) for li in range(len(names))])
    out = {'classes': {n: {k: cols[k][li] for k in KEYS} for li, n in enumerate(names)},
           'coverage_counts': {k: np.array(v, np.int64) for k, v in cnt.items()}}
    for k in KEYS:
        v = np.array(cols[k], np.float64)
        out['all_' + k] = NAN if np.isnan(v).all() else np.nanmean(v)
    return out


def same_bits(a, b, what=''):
    a, b = float(a), float(b)
    if math.isnan(a) or math.isnan(b):
        assert math.isnan(a) and math.isnan(b), (what, a, b)
    else:
        assert a.hex() == b.hex(), (what, a, b)


def assert_coverage_equal(got, want):
    """got: avgs of the evaluator; want: avgs of another evaluation or the brute force's dict"""
    for k in KEYS:
        same_bits(got['all_' + k], want['all_' + k], 'all_' + k)
        for name in want['classes']:
            same_bits(got['classes'][name][k], want['classes'][name][k], (name, k))
    assert set(got['coverage_counts']) == set(TALLIES)
    for k in TALLIES:
        g = got['coverage_counts'][k]
        assert isinstance(g, np.ndarray) and g.dtype == np.int64
        assert np.array_equal(g, want['coverage_counts'][k]), (k, g, want['coverage_counts'][k])


_BRUTE = {}


def brute_of_cases(name, iou_thr, score_thr):
    """computed once per (config, parameters) on the RLE form (the dense form holds the same masks)"""
    key = (name, iou_thr, score_thr)
    if key not in _BRUTE:
        pl, gl = inst_eval_cases.cases(as_rle=True)
        _BRUTE[key] = brute_force(pl, gl, CLASSES, iou_thr=iou_thr, score_thr=score_thr,
                                  **inst_eval_cases.CONFIGS[name])
    return _BRUTE[key]


# ------------------------------------------------------------------------------------------ host path
@pytest.mark.parametrize('iou_thr,score_thr', PARAMS)
@pytest.mark.parametrize('name', sorted(inst_eval_cases.CONFIGS))
@pytest.mark.parametrize('as_rle', [True, False])
def test_host_path_equals_the_brute_force(as_rle, name, iou_thr, score_thr):
    pl, gl = inst_eval_cases.cases(as_rle=as_rle)
    want = brute_of_cases(name, iou_thr, score_thr)
    ev = ScanNetEval(CLASSES, device='cpu', coverage=dict(iou_thr=iou_thr, score_thr=score_thr),
                     **inst_eval_cases.CONFIGS[name])
    assert_coverage_equal(ev.evaluate(pl, gl, verbose=False), want)
    ev.reset()
    for preds, gts in zip(pl, gl):
        ev.update(preds, gts)
    assert_coverage_equal(ev.compute(), want)
    assert ev.last_backend == 'host'


def test_dense_and_rle_cases_give_the_same_brute_force():
    a = brute_force(*inst_eval_cases.cases(as_rle=False), CLASSES)
    assert_coverage_equal(a, brute_of_cases('class_aware', 0.5, 0.0))


def test_coverage_true_is_the_default_parameters():
    pl, gl = inst_eval_cases.cases()
    ev = ScanNetEval(CLASSES, device='cpu', coverage=True)
    assert ev.coverage == dict(iou_thr=0.5, score_thr=0.0)
    assert_coverage_equal(ev.evaluate(pl, gl, verbose=False), brute_of_cases('class_aware', 0.5, 0.0))
    with pytest.raises(ValueError):
        ScanNetEval(CLASSES, coverage=dict(iou=0.5))


def test_anchors_of_the_class_aware_default():
    """the cases keep what makes them worth running: the brute force's own tallies are pinned"""
    detail = []
    pl, gl = inst_eval_cases.cases()
    b = brute_force(pl, gl, CLASSES, detail=detail)
    c = b['coverage_counts']
    assert int(c['tp'].sum()) == 17 and int(c['fp'].sum()) == 18 and int(c['n_gt'].sum()) == 37
    assert sum(1 for ov in detail if ov == 0.5) == 1           # exactly at the threshold: a tp (>=)
    assert int(((c['tp'] > 0) & (c['fp'] > 0)).sum()) == 7
    prec = np.array([b['classes'][n]['prec'] for n in CLASSES])
    assert int(np.isnan(prec).sum()) == 8
    # scan 0: the prediction over two GTs at IoU 0.5 each; all three count
    b0 = brute_force(pl[:1], gl[:1], CLASSES)
    li = 2                                                     # class 3
    assert b0['coverage_counts']['gt_hit'][li] == 3 and b0['coverage_counts']['n_gt'][li] == 3
    assert b0['coverage_counts']['tp'][li] == 2 and b0['coverage_counts']['fp'][li] == 0
    above = brute_force(pl[:1], gl[:1], CLASSES, iou_thr=math.nextafter(0.5, 1.0))
    assert above['coverage_counts']['gt_hit'][li] == 1 and above['coverage_counts']['tp'][li] == 1


def test_recall_is_counted_on_the_gt_side():
    """duplicates make the prediction-side count exceed n_gt for one label; rec stays within [0, 1]"""
    b = brute_of_cases('class_aware', 0.5, 0.0)
    c = b['coverage_counts']
    assert int((c['tp'] > c['n_gt']).sum()) == 1
    rec = np.array([b['classes'][n]['rec'] for n in CLASSES])
    assert np.nanmax(rec) <= 1.0 and (c['gt_hit'] <= c['n_gt']).all()


def test_all_labels_nan_without_a_warning():
    import warnings
    ev = ScanNetEval(CLASSES, device='cpu', coverage=True)
    with warnings.catch_warnings():
        warnings.simplefilter('error')                         # (the AP averages of no scans at all do warn)
        avgs = ev.add_coverage_averages({'classes': {n: {} for n in CLASSES}}, *ev.coverage_of_matches({}))
        for k in KEYS:
            assert math.isnan(avgs['all_' + k])
        assert all(int(v.sum()) == 0 for v in avgs['coverage_counts'].values())


# ------------------------------------------------------------------------------------------ defaults stay
def _flat(d, prefix=''):
    for k, v in d.items():
        if isinstance(v, dict):
            yield from _flat(v, prefix + k + '/')
        else:
            yield prefix + k, float(v).hex() if not math.isnan(float(v)) else 'nan'


@pytest.mark.parametrize('name', sorted(inst_eval_cases.CONFIGS))
def test_coverage_none_changes_nothing(name, capsys):
    pl, gl = inst_eval_cases.cases()
    cfg = inst_eval_cases.CONFIGS[name]
    plain = ScanNetEval(CLASSES, device='cpu', **cfg).evaluate(pl, gl, verbose=True)
    text = capsys.readouterr().out
    for off in (None, False):
        ev = ScanNetEval(CLASSES, device='cpu', coverage=off, **cfg)
        assert ev.coverage is None
        got = ev.evaluate(pl, gl, verbose=True)
        assert capsys.readouterr().out == text and 'mCov' not in text
        assert list(_flat(got)) == list(_flat(plain))          # key for key, bit for bit
        ev.reset()
        for preds, gts in zip(pl, gl):
            ev.update(preds, gts)
        assert list(_flat(ev.compute())) == list(_flat(plain))
    on = ScanNetEval(CLASSES, device='cpu', coverage=True, **cfg).evaluate(pl, gl, verbose=False)
    rest = {k: v for k, v in on.items() if not k.startswith(('all_cov', 'all_wcov', 'all_prec', 'all_rec'))
            and k != 'coverage_counts'}
    rest['classes'] = {n: {k: v for k, v in c.items() if k not in KEYS} for n, c in on['classes'].items()}
    assert list(_flat(rest)) == list(_flat(plain))             # the AP figures are untouched by the option


def test_second_table_is_printed_only_when_on(capsys):
    pl, gl = inst_eval_cases.cases()
    ev = ScanNetEval(CLASSES, device='cpu', coverage=True)
    avgs = ev.evaluate(pl, gl, verbose=True)
    out = capsys.readouterr().out
    assert 'AP_50%' in out and all(c in out for c in ('mCov', 'mWCov', 'mPrec', 'mRec'))
    assert out.index('AP_50%') < out.index('mCov')
    ev.evaluate(pl, gl, verbose=False)
    assert capsys.readouterr().out == ''
    plain = {k: v for k, v in avgs.items() if k != 'all_cov'}
    ev.print_results(plain)                                    # decided by the keys, not by the evaluator
    assert 'mCov' not in capsys.readouterr().out


def test_write_result_file_is_the_benchmark_format(tmp_path):
    pl, gl = inst_eval_cases.cases()
    a = ScanNetEval(CLASSES, device='cpu')
    b = ScanNetEval(CLASSES, device='cpu', coverage=True)
    a.write_result_file(a.evaluate(pl, gl, verbose=False), tmp_path / 'a.csv')
    b.write_result_file(b.evaluate(pl, gl, verbose=False), tmp_path / 'b.csv')
    assert (tmp_path / 'a.csv').read_text() == (tmp_path / 'b.csv').read_text()
