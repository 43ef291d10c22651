"""Runs the REFERENCE's own evaluator (softgroup/evaluation/instance_eval.py, imported from where it
lies, exactly as make_eval_golden.py does; authoring container only) on the inputs of
inst_eval_cases.py and stores its averages -> tests/golden/inst_eval_golden.json.  Every case must
evaluate without raising: the device path's tests rely on the reference alone needing no fallback."""
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import inst_eval_cases  # noqa: E402
from oracle import facade  # noqa: E402


def main():
    np.float, np.bool = float, bool
    import types
    ply = types.ModuleType('plyfile')          # instance_eval_util imports it for file export only
    ply.PlyData = ply.PlyElement = object
    sys.modules.setdefault('plyfile', ply)
    facade.import_reference()
    ref = importlib.import_module('softgroup.evaluation.instance_eval')
    out = {}
    for name, kw in inst_eval_cases.CONFIGS.items():
        ev = ref.ScanNetEval(list(inst_eval_cases.CLASSES), **kw)
        pl, gl = inst_eval_cases.cases()
        assert all(3000 <= len(g) <= 5000 and len(p) <= 40 for p, g in zip(pl, gl))
        avgs = ev.evaluate(pl, gl)
        out[name] = json.loads(json.dumps(avgs, default=float))
    json.dump(out, open(os.path.join(HERE, 'inst_eval_golden.json'), 'w'), indent=1, sort_keys=True)
    print({k: (v['all_ap'], v['all_ap_50%'], v['all_ap_25%']) for k, v in out.items()})


if __name__ == '__main__':
    main()
