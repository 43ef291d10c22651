"""CPU side of the fused optimizer step (softgroup_amd/optim.py, csrc/optim.hip): the switch of
build_optimizer, the torch fallback of the fused classes (bit-equal to the parent class),
state-dict interchange with the stock classes, and the host code of the C ABI (sg_optim_plan, the
argument checks of every entry)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from softgroup_amd import _lib
from softgroup_amd import optim as O
from softgroup_amd.util import build_optimizer


def _model(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.ReLU(), torch.nn.Linear(5, 3))


def test_build_optimizer_switch(monkeypatch):
    m = _model()
    monkeypatch.delenv('SG_FUSED_OPTIM', raising=False)
    for name in ('Adam', 'AdamW', 'SGD'):
        assert type(build_optimizer(m, dict(type=name, lr=0.01))) is getattr(torch.optim, name)
        assert type(build_optimizer(m, dict(type=name, lr=0.01), fused=True)) is O.FUSED_CLASSES[name]
        assert isinstance(build_optimizer(m, dict(type=name, lr=0.01), fused=True), getattr(torch.optim, name))
    monkeypatch.setenv('SG_FUSED_OPTIM', '1')
    assert type(build_optimizer(m, dict(type='Adam', lr=0.01))) is O.FusedAdam
    assert type(build_optimizer(m, dict(type='Adam', lr=0.01), fused=False)) is torch.optim.Adam
    # a type without a fused class is torch's, unchanged
    assert type(build_optimizer(m, dict(type='RMSprop', lr=0.01), fused=True)) is torch.optim.RMSprop
    monkeypatch.setenv('SG_FUSED_OPTIM', '0')
    assert type(build_optimizer(m, dict(type='SGD', lr=0.01))) is torch.optim.SGD
    # only parameters that require a gradient, like the reference
    m[0].bias.requires_grad_(False)
    opt = build_optimizer(m, dict(type='SGD', lr=0.01), fused=True)
    assert len(opt.param_groups[0]['params']) == 3


CASES = [('Adam', dict(lr=0.01)), ('AdamW', dict(lr=0.01, weight_decay=0.01)),
         ('SGD', dict(lr=0.01, momentum=0.9, nesterov=True))]


def _grads(model, step):
    g = torch.Generator().manual_seed(100 + step)
    return [torch.randn(p.shape, generator=g) for p in model.parameters()]


@pytest.mark.parametrize('name,kw', CASES)
def test_cpu_parameters_take_the_parent_step_bit_for_bit(name, kw):
    a, b = _model(), _model()
    fused = build_optimizer(a, dict(type=name, **kw), fused=True)
    stock = build_optimizer(b, dict(type=name, **kw), fused=False)
    for step in range(3):
        for model in (a, b):
            for p, g in zip(model.parameters(), _grads(model, step)):
                p.grad = g.clone()
        fused.step()
        stock.step()
        for p, q in zip(a.parameters(), b.parameters()):
            assert torch.equal(p, q)
    sa, sb = fused.state_dict(), stock.state_dict()
    assert sa['param_groups'] == sb['param_groups']
    for k, st in sb['state'].items():
        assert set(sa['state'][k]) == set(st)
        for key, v in st.items():
            assert torch.equal(sa['state'][k][key], v), (k, key)


@pytest.mark.parametrize('name,kw', CASES)
def test_state_dict_interchange_and_lr_edits(name, kw):
    """stock -> fused -> stock after steps: the continued runs stay bit-equal to a run that never
    changed class, and an edit of param_group['lr'] (cosine_lr_after_step) is honoured"""
    cls, fcls = getattr(torch.optim, name), O.FUSED_CLASSES[name]
    ref_model, model = _model(), _model()
    ref = cls(ref_model.parameters(), **kw)
    opt = cls(model.parameters(), **kw)
    for step in range(6):
        if step in (2, 4):        # hand over through a checkpoint, as checkpoint_save / load_checkpoint do
            sd = copy.deepcopy(opt.state_dict())
            opt = (fcls if step == 2 else cls)(model.parameters(), **kw)
            opt.load_state_dict(sd)
            assert set(opt.state_dict()['state'][0]) == set(ref.state_dict()['state'][0])
        lr = 0.01 * (0.5 ** step)
        for o in (ref, opt):
            for g in o.param_groups:
                g['lr'] = lr
        for m in (ref_model, model):
            for p, g in zip(m.parameters(), _grads(m, step)):
                p.grad = g.clone()
        ref.step()
        opt.step()
        for p, q in zip(ref_model.parameters(), model.parameters()):
            assert torch.equal(p, q), step
    # the lr edits did something
    assert opt.param_groups[0]['lr'] == 0.01 * 0.5 ** 5


def test_grad_none_is_skipped_and_amp_attribute():
    m = _model()
    opt = O.FusedAdam(m.parameters(), lr=0.1)
    assert opt._step_supports_amp_scaling and opt.clip_grad_norm is None and opt.last_grad_norm is None
    before = [p.detach().clone() for p in m.parameters()]
    m[0].weight.grad = torch.ones_like(m[0].weight)
    opt.step()
    after = list(m.parameters())
    assert not torch.equal(before[0], after[0])
    for b, a in zip(before[1:], after[1:]):
        assert torch.equal(b, a)


# ---- the C ABI's host code --------------------------------------------------------------------
def _restated_plan(counts, chunk):
    out = []
    for t, n in enumerate(counts):
        for off in range(0, n, chunk):
            out.append((t, off, min(chunk, n - off)))
    return np.array(out, dtype=np.int64).reshape(-1, 3)


def test_plan_covers_every_element_once():
    chunk = O.chunk_elems()
    assert chunk > 0 and chunk % 4 == 0
    counts = [0, 1, 3, chunk - 1, chunk, chunk + 1, 3 * chunk + 1] + [5] * 700
    chunks = O.plan_chunks(counts)
    assert np.array_equal(chunks, _restated_plan(counts, chunk))
    # restated as properties: in order, every element exactly once, no chunk across a tensor
    covered = [0] * len(counts)
    last = (-1, 0)
    for t, off, n in chunks.tolist():
        assert 0 < n <= chunk and (t, off) > last
        assert off == covered[t] and off + n <= counts[t]
        covered[t] += n
        last = (t, off)
    assert covered == counts
    assert len(O.plan_chunks([])) == 0 and len(O.plan_chunks([0, 0])) == 0


def test_plan_bad_arguments():
    lib = _lib.lib()
    counts = np.array([4, -1], dtype=np.int64)
    out = np.zeros((4, 3), dtype=np.int64)
    for rc in (lib.sg_optim_plan(counts.ctypes.data, 2, None, 0),          # negative count
               lib.sg_optim_plan(None, 2, None, 0),                        # null counts
               lib.sg_optim_plan(counts.ctypes.data, -1, None, 0),
               lib.sg_optim_plan(counts.ctypes.data, 1, None, 4)):         # null chunks with a capacity
        assert rc < 0 and b'sg_optim_plan' in lib.sg_last_error()
    big = np.array([10 * O.chunk_elems()], dtype=np.int64)
    rc = lib.sg_optim_plan(big.ctypes.data, 1, out.ctypes.data, 4)         # 10 chunks into room for 4
    assert rc < 0 and b'sg_optim_plan' in lib.sg_last_error()
    assert lib.sg_optim_plan(big.ctypes.data, 1, None, 0) == 10


def test_entries_reject_bad_arguments_without_a_launch():
    """negative counts and null tables with chunks: < 0 and the entry's name, before anything touches
    the device (this runs without one)"""
    lib = _lib.lib()
    buf = (C.c_int64 * 8)()
    p = C.addressof(buf)
    hyper = (0.01, 0.9, 0.999, 1e-8, 0.0)
    calls = {
        'sg_optim_grad_norm': [
            lambda: lib.sg_optim_grad_norm(None, 1, None, 3, None, 1.0, p, p, 1 << 20, None),
            lambda: lib.sg_optim_grad_norm(p, -1, p, 1, None, 1.0, p, p, 1 << 20, None),
            lambda: lib.sg_optim_grad_norm(p, 1, p, -2, None, 1.0, p, p, 1 << 20, None),
            lambda: lib.sg_optim_grad_norm(p, 1, p, 1, None, -1.0, p, p, 1 << 20, None),
            lambda: lib.sg_optim_grad_norm(p, 1, p, 1, None, 1.0, None, p, 1 << 20, None),
            lambda: lib.sg_optim_grad_norm(p, 1, p, 1, None, 1.0, p, p, 8, None),
        ],
        'sg_optim_adam_step': [
            lambda: lib.sg_optim_adam_step(None, 1, None, 3, *hyper, 0, None, None, None, 0, p, None),
            lambda: lib.sg_optim_adam_step(p, 1, p, -1, *hyper, 0, None, None, None, 0, p, None),
            lambda: lib.sg_optim_adam_step(p, 1, p, 1, 0.01, 1.5, 0.999, 1e-8, 0.0, 0, None, None, None, 0, p, None),
            lambda: lib.sg_optim_adam_step(p, 1, p, 1, *hyper, 0, None, None, None, 0, None, None),
        ],
        'sg_optim_sgd_step': [
            lambda: lib.sg_optim_sgd_step(None, 1, None, 3, 0.01, 0.9, 0.0, 0.0, 0, None, None, None, 0, p, None),
            lambda: lib.sg_optim_sgd_step(p, -1, p, 1, 0.01, 0.9, 0.0, 0.0, 0, None, None, None, 0, p, None),
            lambda: lib.sg_optim_sgd_step(p, 1, p, 1, 0.01, 0.0, 0.0, 0.0, 1, None, None, None, 0, p, None),
        ],
        'sg_optim_scale_grads': [
            lambda: lib.sg_optim_scale_grads(None, 1, None, 3, p, None),
            lambda: lib.sg_optim_scale_grads(p, 1, p, -1, p, None),
            lambda: lib.sg_optim_scale_grads(p, 1, p, 1, None, None),
        ],
    }
    for name, fns in calls.items():
        for i, fn in enumerate(fns):
            rc = fn()
            assert rc < 0 and name.encode() in lib.sg_last_error(), (name, i, rc, lib.sg_last_error())
    # an empty tensor list is a valid call and launches nothing
    assert lib.sg_optim_grad_norm(None, 0, None, 0, None, 1.0, p, p, 1 << 20, None) == 0
    assert lib.sg_optim_adam_step(None, 0, None, 0, *hyper, 1, None, None, None, 0, None, None) == 0
    assert lib.sg_optim_sgd_step(None, 0, None, 0, 0.01, 0.9, 0.0, 0.0, 0, None, None, None, 0, None, None) == 0
    assert lib.sg_optim_scale_grads(None, 0, None, 0, p, None) == 0
    assert lib.sg_optim_workspace_bytes() >= 16
