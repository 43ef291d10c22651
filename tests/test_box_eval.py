"""Box detection AP (softgroup_amd.evaluation.det_eval), numpy path: against the reference's
tools/eval_det.py outputs stored in box_eval_golden.json -- get_iou, voc_ap, eval_det_cls, eval_det
(with its KeyError), eval_sphere and evaluate_box_ap on small scans -- bit for bit, with the key order,
a custom get_iou_func and the tool's file reading."""
import json
import os
import sys
import warnings

import numpy as np
import pytest

from softgroup_amd.evaluation import det_eval as de
from softgroup_amd.evaluation import eval_det, eval_det_cls, eval_sphere, evaluate_box_ap, get_iou, voc_ap

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import box_eval_cases as bc  # noqa: E402

GOLD = json.load(open(os.path.join(HERE, 'golden', 'box_eval_golden.json')))


def same(a, b):
    """exact equality of floats / lists of floats, NaN equal to NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def check_res(res, gold):
    rec, prec, ap = res
    assert list(ap) == gold['keys'] and list(rec) == gold['keys'] and list(prec) == gold['keys']
    for k, r, p, a in zip(gold['keys'], gold['rec'], gold['prec'], gold['ap']):
        assert same(rec[k], r) and same(prec[k], p) and same(ap[k], a), k
        if isinstance(a, int):                      # eval_sphere's 0 for a class without predictions
            assert isinstance(ap[k], int) and isinstance(rec[k], int)


def check_det(name, device):
    pred_all, gt_all = bc.det_cases()[name]
    for key, g in GOLD['det'][name].items():
        t, u07 = key.split('_')
        t, u07 = float(t), bool(int(u07))
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            if 'KeyError' in g['eval_det']:
                with pytest.raises(KeyError) as e:
                    eval_det(pred_all, gt_all, t, u07, device=device)
                assert e.value.args[0] == g['eval_det']['KeyError']
            else:
                check_res(eval_det(pred_all, gt_all, t, u07, device=device), g['eval_det'])
            check_res(eval_sphere(pred_all, gt_all, t, u07, device=device), g['eval_sphere'])


def check_cls(device):
    pred_all, gt_all = bc.det_cases()['random']
    pred = {img: [(b, s) for c, b, s in p if c == 'chair'] for img, p in pred_all.items()}
    gt = {img: [b for c, b in g if c == 'chair'] for img, g in gt_all.items()}
    for t in bc.THRESHOLDS:
        for name, p in ((f'random_chair_{t}', pred), (f'empty_{t}', {})):
            rec, prec, ap = eval_det_cls(p, gt, t, device=device)
            g = GOLD['cls'][name]
            assert same(rec, g['rec']) and same(prec, g['prec']) and same(ap, g['ap']), name


def scene_inputs(name):
    coords, masks, sems, insts, labels, confs = bc.scene_cases()[name]
    preds = [[dict(scan_id=f'scan{s}', label_id=lab, conf=c, pred_mask=m)
              for m, lab, c in zip(masks[s], labels[s], confs[s])] for s in range(len(coords))]
    return preds, coords, sems, insts


def check_scene(name, device):
    preds, coords, sems, insts = scene_inputs(name)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        res = evaluate_box_ap(preds, coords, sems, insts, bc.CLASSES, device=device)
    assert list(res) == list(bc.THRESHOLDS)
    for t in bc.THRESHOLDS:
        g = GOLD['scenes'][name][str(t)]
        check_res((res[t]['rec'], res[t]['prec'], res[t]['ap']), g)
        assert same(res[t]['mAP'], g['mAP'])


def test_get_iou_and_voc_ap_equal_reference():
    for (a, b), g in zip(bc.iou_pairs(), GOLD['iou']):
        assert same(get_iou(a, b), g)
        assert same(de._iou_rows(a, b[None])[0], g)
    for (rec, prec), (g0, g1) in zip(bc.voc_inputs(), GOLD['voc']):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            assert same(voc_ap(rec, prec), g0) and same(voc_ap(rec, prec, True), g1)


@pytest.mark.parametrize('name', sorted(GOLD['det']))
def test_eval_det_and_sphere_numpy_equal_reference(name):
    check_det(name, 'cpu')


def test_eval_det_cls_numpy_equals_reference():
    check_cls('cpu')


@pytest.mark.parametrize('name', sorted(GOLD['scenes']))
def test_evaluate_box_ap_numpy_equals_reference(name):
    check_scene(name, 'cpu')


def test_eval_det_raises_key_error_for_gt_class_without_predictions():
    pred_all, gt_all = bc.det_cases()['gt_class_without_pred']
    with pytest.raises(KeyError):
        eval_det(pred_all, gt_all, device='cpu')
    rec, prec, ap = eval_sphere(pred_all, gt_all, device='cpu')
    assert list(ap) == ['chair', 'sofa'] and ap['sofa'] == 0 and rec['sofa'] == 0


def test_custom_get_iou_func_is_called_per_pair():
    pred_all, gt_all = bc.det_cases()['random']
    calls = []

    def iou(a, b):
        calls.append(1)
        return get_iou(a, b)
    ref = eval_sphere(pred_all, gt_all, 0.25, device='cpu')
    got = eval_sphere(pred_all, gt_all, 0.25, get_iou_func=iou, device='cpu')
    assert calls
    for k in ref[2]:
        assert same(ref[0][k], got[0][k]) and same(ref[1][k], got[1][k]) and same(ref[2][k], got[2][k])

    # a different IoU changes the result: (a constant 1 makes every first detection of a GT a TP)
    ones = eval_sphere(pred_all, gt_all, 0.5, get_iou_func=lambda a, b: 1.0, device='cpu')
    assert any(not same(ones[2][k], ref[2][k]) for k in ref[2])


def test_box_extraction_numpy_rle_equals_dense():
    from softgroup_amd.util.rle import rle_encode
    preds, coords, sems, insts = scene_inputs('f32')
    rle = [[dict(p, pred_mask=rle_encode(p['pred_mask'])) for p in ps] for ps in preds]
    a = evaluate_box_ap(preds, coords, sems, insts, bc.CLASSES, device='cpu')
    b = evaluate_box_ap(rle, coords, sems, insts, bc.CLASSES, device='cpu')
    for t in a:
        assert same(a[t]['mAP'], b[t]['mAP'])


def test_empty_instance_id_raises_index_error():
    preds, coords, sems, insts = scene_inputs('f64_negative')
    insts = [i.copy() for i in insts]
    insts[1][insts[1] == 2] = -100
    with pytest.raises(IndexError):
        evaluate_box_ap(preds, coords, sems, insts, bc.CLASSES, device='cpu')
