"""Runs the REFERENCE's tools/eval_det.py (imported by path; authoring container only) on the inputs of
box_eval_cases.py and stores its outputs -> tests/golden/box_eval_golden.json: get_iou, voc_ap (both
metrics), eval_det_cls, eval_det (or the KeyError it raises) and eval_sphere at 0.25 and 0.5 with both
AP metrics, and the eval_sphere results of small scans whose boxes are formed as the script's
__main__ forms them (coords[mask].min(0) / .max(0), GT class from the instance's first point).

numpy's default argsort is not stable, so every case is also run with a stable sort and with ties in
reverse index order; the generator refuses a case whose result depends on the tie order."""
import importlib.util
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import box_eval_cases as bc  # noqa: E402

REF = '/root/reference/tools/eval_det.py'


class _TieOrder:
    """numpy with argsort's tie order replaced ('stable' or 'reverse'), for the reference module"""

    def __init__(self, mode):
        self.mode = mode

    def __getattr__(self, name):
        return getattr(np, name)

    def argsort(self, a, **kw):
        a = np.asarray(a)
        if self.mode == 'stable':
            return np.argsort(a, kind='stable')
        return np.lexsort((-np.arange(len(a)), a))


def _num(x):
    if isinstance(x, np.ndarray):
        return [float(v) for v in x.reshape(-1)]
    return x if isinstance(x, int) else float(x)


def _enc(res):
    rec, prec, ap = res
    return {'keys': list(ap.keys()), 'rec': [_num(rec[k]) for k in ap], 'prec': [_num(prec[k]) for k in ap],
            'ap': [_num(ap[k]) for k in ap]}


def _same(a, b):
    return json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)


def _scene_sets(case):
    """eval_det.py __main__'s pred_all / gt_all for the scans of a scene case"""
    coords, masks, sems, insts, labels, confs = case
    pred_all, gt_all = {}, {}
    for s in range(len(coords)):
        pred = []
        for m, lab, conf in zip(masks[s], labels[s], confs[s]):
            pts = coords[s][np.asarray(m).astype(bool)]
            pred.append((bc.CLASSES[lab - 1], np.concatenate([pts.min(0), pts.max(0)]), conf))
        gt = []
        for i in range(int(insts[s].max()) + 1):
            sel = insts[s] == i
            cls_id = int(sems[s][np.nonzero(sel)[0][0]])
            if cls_id >= 2:
                pts = coords[s][sel]
                gt.append((bc.CLASSES[cls_id - 2], np.concatenate([pts.min(0), pts.max(0)])))
        pred_all[s], gt_all[s] = pred, gt
    return pred_all, gt_all


def run(ref):
    out = {'iou': [], 'voc': [], 'det': {}, 'cls': {}, 'scenes': {}}
    for a, b in bc.iou_pairs():
        out['iou'].append(float(ref.get_iou(a, b)))
    for rec, prec in bc.voc_inputs():
        out['voc'].append([float(ref.voc_ap(rec, prec, False)), float(ref.voc_ap(rec, prec, True))])
    for name, (pred_all, gt_all) in bc.det_cases().items():
        r = {}
        for t in bc.THRESHOLDS:
            for u07 in (False, True):
                key = f'{t}_{int(u07)}'
                try:
                    det = _enc(ref.eval_det(pred_all, gt_all, t, u07))
                except KeyError as e:
                    det = {'KeyError': e.args[0]}
                r[key] = {'eval_det': det, 'eval_sphere': _enc(ref.eval_sphere(pred_all, gt_all, t, u07))}
        out['det'][name] = r
    # eval_det_cls directly: one class of the random case, and an empty prediction map
    pred_all, gt_all = bc.det_cases()['random']
    pred = {img: [(b, s) for c, b, s in p if c == 'chair'] for img, p in pred_all.items()}
    gt = {img: [b for c, b in g if c == 'chair'] for img, g in gt_all.items()}
    for t in bc.THRESHOLDS:
        rec, prec, ap = ref.eval_det_cls(pred, gt, t)
        out['cls'][f'random_chair_{t}'] = {'rec': _num(rec), 'prec': _num(prec), 'ap': _num(ap)}
        rec, prec, ap = ref.eval_det_cls({}, gt, t)
        out['cls'][f'empty_{t}'] = {'rec': _num(rec), 'prec': _num(prec), 'ap': _num(ap)}
    for name, case in bc.scene_cases().items():
        pred_all, gt_all = _scene_sets(case)
        r = {}
        for t in bc.THRESHOLDS:
            res = ref.eval_sphere(pred_all, gt_all, ovthresh=t)
            r[str(t)] = dict(_enc(res), mAP=float(np.mean(list(res[-1].values()))))
        out['scenes'][name] = r
    return out


def main():
    warnings.simplefilter('ignore', RuntimeWarning)           # npos = 0: the reference's 0 / 0
    spec = importlib.util.spec_from_file_location('ref_eval_det', REF)
    ref = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = ref                              # (eval_sphere's pool pickles by module name)
    spec.loader.exec_module(ref)
    gold = run(ref)
    for mode in ('stable', 'reverse'):
        ref.np = _TieOrder(mode)
        other = run(ref)
        ref.np = np
        for part in ('det', 'cls', 'scenes'):
            for name in gold[part]:
                assert _same(gold[part][name], other[part][name]), (mode, part, name)
    path = os.path.join(HERE, 'box_eval_golden.json')
    json.dump(gold, open(path, 'w'), indent=1, sort_keys=True)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
