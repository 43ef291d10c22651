"""Runs the REFERENCE's own point-wise evaluators and PanopticEval
(/root/reference/softgroup/evaluation/point_wise_eval.py and panoptic_eval.py, imported from where
they lie; authoring container only) on the deterministic inputs of pointwise_cases.py and stores
their outputs -> tests/golden/pointwise_golden.json: returned figures, logged lines, the printed
panoptic table and evaluate_single's per-scan arrays.
numpy >= 1.24 dropped np.float, which the reference still uses: aliased for the run.  Instance
labels stay int64: numpy 2 refuses int32 * 2**32."""
import contextlib
import importlib
import io
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import pointwise_cases as pc  # noqa: E402
from oracle import facade  # noqa: E402


class Capture:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


def _f(x):
    return [float(v) for v in np.asarray(x, np.float64).reshape(-1)] if np.ndim(x) else float(x)


def main():
    np.float = float
    warnings.simplefilter('ignore', RuntimeWarning)           # 0 / 0 of the all-ignored case
    facade.import_reference()
    pw = importlib.import_module('softgroup.evaluation.point_wise_eval')
    pe = importlib.import_module('softgroup.evaluation.panoptic_eval')
    out = {'semantic': {}, 'panoptic': {}}
    for name, (sp, sg, op, og, inst) in pc.semantic_cases().items():
        log = Capture()
        r = dict(miou=_f(pw.evaluate_semantic_miou(sp, sg, pc.IGNORE, log)),
                 acc=_f(pw.evaluate_semantic_acc(sp, sg, pc.IGNORE, log)),
                 mae=_f(pw.evaluate_offset_mae(op, og, inst, pc.IGNORE, log)))
        r['log'] = log.lines
        out['semantic'][name] = r
    keys = ('PQ', 'PQ_dagger', 'SQ', 'RQ', 'IoU', 'pq_all', 'pq_dagger_all', 'sq_all', 'rq_all', 'iou_all')
    single = ('pan_tp', 'pan_iou', 'pan_fp', 'pan_fn', 'seen', 'correct', 'positive')
    for name, (thing, stuff, kw, preds, sems, insts) in pc.panoptic_cases().items():
        ev = pe.PanopticEval(thing, stuff, **kw)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            res = ev.evaluate(preds, sems, [i.astype(np.int64) for i in insts])
        r = {k: _f(v) for k, v in zip(keys, res)}
        r['table'] = buf.getvalue()
        r['single'] = [{k: _f(v) for k, v in zip(single, ev.evaluate_single(p, s, i.astype(np.int64).copy()))}
                       for p, s, i in zip(preds, sems, insts)]
        out['panoptic'][name] = r
    json.dump(out, open(os.path.join(HERE, 'pointwise_golden.json'), 'w'), indent=1, sort_keys=True)
    print({k: (v['miou'], v['acc'], v['mae']) for k, v in out['semantic'].items()})
    print({k: (v['PQ'], v['IoU']) for k, v in out['panoptic'].items()})


if __name__ == '__main__':
    main()
