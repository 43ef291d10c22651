"""ScanNetEval's backend keyword and streaming form (reset / update / compute) on the host backend
against the averages the REFERENCE's evaluator produced on tests/golden/inst_eval_cases.py
(inst_eval_golden.json, from make_inst_eval_golden.py), and the C ABI of the device path.  The device
path itself is checked in tests/test_inst_eval_gpu.py."""
import ctypes
import json
import math
import os
import re
import sys

import pytest

from softgroup_amd import _lib
from softgroup_amd.evaluation import ScanNetEval

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import inst_eval_cases  # noqa: E402

GOLD = json.load(open(os.path.join(HERE, 'golden', 'inst_eval_golden.json')))
SYMBOLS = ('sg_inst_rle_run_slots', 'sg_inst_rle_parse', 'sg_inst_scan_workspace_bytes', 'sg_inst_scan_update',
           'sg_inst_curves_workspace_bytes', 'sg_inst_curves')


def _same(a, b):
    if isinstance(b, dict):
        assert set(a) == set(b)
        for k in b:
            _same(a[k], b[k])
    else:
        a, b = float(a), float(b)
        assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-12, (a, b)


@pytest.mark.parametrize('name', sorted(inst_eval_cases.CONFIGS))
@pytest.mark.parametrize('as_rle', [True, False])
def test_host_backend_equals_the_reference(name, as_rle):
    pl, gl = inst_eval_cases.cases(as_rle=as_rle)
    ev = ScanNetEval(list(inst_eval_cases.CLASSES), device='cpu', **inst_eval_cases.CONFIGS[name])
    for backend in (None, 'host'):
        _same(ev.evaluate(pl, gl, verbose=False, backend=backend), GOLD[name])
        assert ev.last_backend == 'host' and ev.last_fallback is None


@pytest.mark.parametrize('name', sorted(inst_eval_cases.CONFIGS))
def test_streaming_form_on_the_host_backend(name, capsys):
    pl, gl = inst_eval_cases.cases()
    ev = ScanNetEval(list(inst_eval_cases.CLASSES), device='cpu', **inst_eval_cases.CONFIGS[name])
    for _ in range(2):                                  # reset() starts over
        ev.reset()
        for preds, gts in zip(pl, gl):
            ev.update(preds, gts)
        _same(ev.compute(), GOLD[name])
        assert ev.last_backend == 'host' and ev.last_fallback is None
    assert capsys.readouterr().out == ''                # compute is quiet unless asked
    ev.compute(verbose=True)
    assert 'AP_50%' in capsys.readouterr().out


def test_cases_stay_small():
    pl, gl = inst_eval_cases.cases()
    assert len(pl) == 5
    for preds, gts in zip(pl, gl):
        assert 3000 <= len(gts) <= 5000 and len(preds) <= 40
        assert len(set(int(g) for g in gts if g >= 1000)) <= 16


def test_device_backend_without_a_gpu_raises():
    import torch
    pl, gl = inst_eval_cases.cases()
    ev = ScanNetEval(list(inst_eval_cases.CLASSES), device='cpu')
    with pytest.raises(RuntimeError, match='needs a GPU'):
        ev.evaluate(pl, gl, verbose=False, backend='device')
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='needs a GPU'):
            ScanNetEval(list(inst_eval_cases.CLASSES)).reset(backend='device')
    with pytest.raises(ValueError):
        ev.evaluate(pl, gl, verbose=False, backend='gpu')


def test_c_symbols_declared_exported_and_bound():
    root = os.path.dirname(HERE)
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'softgroup_hip.h')).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % s, hdr), s
        assert hasattr(raw, s), s
        assert s in _lib.SIGNATURES, s
    lib = _lib.lib()
    assert lib.sg_inst_rle_run_slots(0, 0) == 1 and lib.sg_inst_rle_run_slots(7, 1) == 3
    # arguments out of range give no size, and a too small workspace its own error code: nothing is launched
    assert lib.sg_inst_scan_workspace_bytes(1000, 4, 10, 18, 0, 10, 18, None) == 0
    assert lib.sg_inst_curves_workspace_bytes(100, 180) > 0
    assert lib.sg_inst_curves(None, None, 0, 1, 180, 1, 1, 1, None, 0, None) == -2
