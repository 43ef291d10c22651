"""The fused optimizer step (csrc/optim.hip, softgroup_amd/optim.py) on the device.

Reference: the formulas of torch's single-tensor Adam / AdamW / SGD evaluated in float64 (numpy)
from the same float32 inputs.  Tolerance: the stock torch optimizer (float32, same device, same
inputs) runs in the same test; its largest error against the float64 result, per quantity, in
units of ulp(float32) of the float64 value, is E.  The fused path may be at most 2 E + 1 ulp: the
factor covers a different but equally valid order of the same few float32 operations, the 1 ulp the
final rounding.  Both figures are printed and written to profiles/optim_parity.txt.

The `*_above_the_launch_caps` cases run the same checks on _sizes_above(): more chunks than one trip of the
norm, step and scale kernels takes (tests/test_launch_caps_train.py pins the list to the caps in the source).
"""
import copy
import math
import os

import numpy as np
import pytest
import torch

from softgroup_amd import optim as O
from softgroup_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 3
_FIGURES = {}


def _record(name, figures):
    """keep the (stock, fused) error figures of a test and rewrite profiles/optim_parity.txt"""
    _FIGURES[name] = figures
    lines = ['# tests/test_fused_optim_gpu.py: largest error against the float64 formulas, in ulp(float32);',
             '# stock = torch.optim on the same device and inputs; bound for fused = 2 * stock + 1',
             f'# device: {torch.cuda.get_device_name(0)}', '']
    for test in sorted(_FIGURES):
        lines.append(test)
        for what, (stock, fused) in _FIGURES[test].items():
            lines.append(f'  {what:<28s} stock {stock:10.4f}   fused {fused:10.4f}')
    try:
        with open(os.path.join(ROOT, 'profiles', 'optim_parity.txt'), 'w') as f:
            f.write('\n'.join(lines) + '\n')
    except OSError:
        pass


def _sizes():
    c = O.chunk_elems()
    return [1, 3, 4, 63, 64, 65, 255, 257, c - 1, c, c + 1, 3 * c + 1, 0] + [5] * 700


def _sizes_above():
    """more chunks than one trip of any kernel takes: above kOptMaxBlocks = 2048 workgroups of the step and scale
    kernels, above twice kOptNormBlocks = 1024 of the norm kernel (a third trip), and the five chunks of the
    4 * c + 1 tensor on both sides of chunk 2048: its `arrive` count is split across two trips of the walk"""
    c = O.chunk_elems()
    return [c + 1, 3 * c + 1] + [5] * 1100 + [1, 63, 257, c - 1] + [5] * 936 + [4 * c + 1, 2 * c, 3]


STEP_CAP, NORM_CAP = 2048, 1024      # kOptMaxBlocks, kOptNormBlocks (tests/test_launch_caps_train.py reads them)
VIEWS = {7: 1, 10: 3}      # tensor index -> element offset of the view into a larger buffer (misaligned start)


def _make_inputs(sizes, seed):
    """float32 parameters (|x| in 1e-3 .. 10, both signs) and STEPS gradient sets (some elements
    exactly 0) as flat numpy arrays plus the tensor sizes.  Never modified."""
    rng = np.random.default_rng(seed)
    n = sum(sizes)
    assert n < 300000
    p = (10.0 ** rng.uniform(-3, 1, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    grads = []
    for _ in range(STEPS):
        g = rng.standard_normal(n).astype(np.float32) * (10.0 ** rng.uniform(-3, 0, n)).astype(np.float32)
        g[rng.random(n) < 0.05] = 0.0
        grads.append(g)
    for a in [p] + grads:
        a.setflags(write=False)
    return dict(sizes=sizes, p=p, grads=grads)


@pytest.fixture(scope='module')
def inputs():
    return _make_inputs(_sizes(), 1234)


@pytest.fixture(scope='module')
def inputs_above():
    return _make_inputs(_sizes_above(), 4321)


def _split(flat, sizes, views=True):
    """device tensors of `sizes` holding `flat`; two of them views at an odd element offset"""
    out, at = [], 0
    dev_flat = torch.from_numpy(np.array(flat)).to(DEV)      # (one upload; the tensors are filled on the device)
    for i, n in enumerate(sizes):
        src = dev_flat[at:at + n]
        at += n
        off = VIEWS.get(i, 0) if views else 0
        buf = torch.zeros(n + off + 8, dtype=torch.float32, device=DEV)
        t = buf[off:off + n]
        t.copy_(src)
        if off:
            assert t.data_ptr() % 16 == 4 * off
        out.append(t)
    return out


def _flat(tensors):
    return torch.cat([t.detach().reshape(-1) for t in tensors]).cpu().numpy()


def _params(inputs):
    return [t.requires_grad_(True) for t in _split(inputs['p'], inputs['sizes'])]


def _set_grads(params, inputs, step, scale=1.0):
    for p, g in zip(params, _split(inputs['grads'][step] * np.float32(scale), inputs['sizes'])):
        p.grad = g


def _ulps(got, ref):
    """largest |got - ref| in units of ulp(float32) at |ref|"""
    ref = np.asarray(ref, dtype=np.float64)
    if ref.size == 0:
        return 0.0
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref) / ulp))


# ---- the formulas in float64 --------------------------------------------------------------------
def _adam64(p, m, v, g, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, adamw=False):
    b1, b2 = betas
    if adamw:
        p = p * (1 - lr * weight_decay)
    elif weight_decay:
        g = g + weight_decay * p
    m = m + (1 - b1) * (g - m)
    v = b2 * v + (1 - b2) * g * g
    p = p - (lr / (1 - b1 ** step)) * m / (np.sqrt(v) / math.sqrt(1 - b2 ** step) + eps)
    return p, m, v


def _sgd64(p, buf, g, step, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
    if weight_decay:
        g = g + weight_decay * p
    if momentum:
        buf = g.copy() if step == 1 else momentum * buf + (1 - dampening) * g
        g = g + momentum * buf if nesterov else buf
    return p - lr * g, buf


CONFIGS = {
    'adam': ('Adam', dict(lr=1e-2)),
    'adamw_wd0.01': ('AdamW', dict(lr=1e-2, weight_decay=0.01)),
    'adam_wd1e-4': ('Adam', dict(lr=1e-2, weight_decay=1e-4)),
    'sgd': ('SGD', dict(lr=1e-2)),
    'sgd_momentum': ('SGD', dict(lr=1e-2, momentum=0.9)),
    'sgd_nesterov_wd': ('SGD', dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-4)),
}


def _reference(inputs, name, kw, coef=None):
    """[(p, state0, state1)] after every step, float64"""
    p = inputs['p'].astype(np.float64)
    s0, s1 = np.zeros_like(p), np.zeros_like(p)
    out = []
    for step in range(1, STEPS + 1):
        g = inputs['grads'][step - 1].astype(np.float64)
        if coef is not None:
            g = g * coef[step - 1]
        if name == 'SGD':
            p, s0 = _sgd64(p, s0, g, step, **kw)
        else:
            p, s0, s1 = _adam64(p, s0, s1, g, step, adamw=name == 'AdamW', **kw)
        out.append((p, s0, s1))
    return out


STATE_KEYS = {'Adam': ('exp_avg', 'exp_avg_sq'), 'AdamW': ('exp_avg', 'exp_avg_sq'), 'SGD': ('momentum_buffer', )}


def _run(inputs, name, kw, fused, before_step=None, all_steps=False):
    """-> per step (p, state0, state1 or None, steps or None) as flat float32 arrays; the counters of a sample
    of the tensors, or of all of them"""
    params = _params(inputs)
    cls = O.FUSED_CLASSES[name] if fused else getattr(torch.optim, name)
    opt = cls(params, **kw)
    live = [p for p in params if p.numel()]
    out = []
    for step in range(STEPS):
        _set_grads(params, inputs, step)
        if before_step is not None:
            before_step(opt, params)
        opt.step()
        states = []
        for key in STATE_KEYS[name]:
            if all(opt.state[p].get(key) is not None for p in live):
                states.append(_flat([opt.state[p][key] for p in live]))
            else:
                states.append(None)
        steps = None
        if 'step' in opt.state[live[0]] and all_steps:
            steps = torch.stack([opt.state[p]['step'].reshape(()).float().to(DEV) for p in live]).cpu().numpy()
            assert steps.shape == (len(live), )
        elif 'step' in opt.state[live[0]]:
            steps = np.array([float(opt.state[p]['step']) for p in live[:40] + live[-3:]])
        out.append((_flat(live), states, steps))
        opt.zero_grad()
    return out


def _steps_against_float64(inputs, config, key, all_steps=False):
    name, kw = CONFIGS[config]
    ref = _reference(inputs, name, kw)
    stock = _run(inputs, name, kw, fused=False)
    fused = _run(inputs, name, kw, fused=True, all_steps=all_steps)
    again = _run(inputs, name, kw, fused=True)
    figures, failures = {}, []
    for step in range(STEPS):
        want = (ref[step][0], ) + tuple(ref[step][1:1 + len(STATE_KEYS[name])])
        got_s = (stock[step][0], ) + tuple(stock[step][1])
        got_f = (fused[step][0], ) + tuple(fused[step][1])
        for what, w, s, f in zip(('p', ) + STATE_KEYS[name], want, got_s, got_f):
            if f is None and s is None:
                continue                        # (SGD without momentum keeps no buffer)
            assert f is not None and s is not None, (what, step)
            es, ef = _ulps(s, w), _ulps(f, w)
            figures[f'step {step + 1} {what}'] = (es, ef)
            print(f'{config} step {step + 1} {what:<16s} stock {es:.4f} ulp   fused {ef:.4f} ulp')
            if not ef <= 2 * es + 1:
                failures.append((step + 1, what, es, ef))
        # the counters: exact
        assert fused[step][2] is not None and np.all(fused[step][2] == step + 1), fused[step][2]
        # two runs of the fused step from the same inputs: the same bits
        assert np.array_equal(fused[step][0], again[step][0])
        for a, b in zip(fused[step][1], again[step][1]):
            assert (a is None and b is None) or np.array_equal(a, b)
    _record(f'{key}[{config}]', figures)
    assert not failures, failures


@pytest.mark.parametrize('config', sorted(CONFIGS))
def test_steps_against_float64(inputs, config):
    _steps_against_float64(inputs, config, 'steps')


def test_sizes_above_reach_a_second_trip_of_every_chunk_walk():
    sizes, c = _sizes_above(), O.chunk_elems()
    chunks = O.plan_chunks(sizes)
    assert len(chunks) > STEP_CAP and len(chunks) > 2 * NORM_CAP and sum(sizes) < 300000
    big = sizes.index(4 * c + 1)
    of_big = np.flatnonzero(chunks[:, 0] == big)
    assert len(of_big) == 5 and of_big[0] < STEP_CAP <= of_big[-1]            # `arrive` counts in two trips
    assert np.array_equal(chunks[of_big, 1], c * np.arange(5)) and chunks[of_big[-1], 2] == 1
    assert all(sizes[i] == 5 for i in VIEWS)                                    # the two misaligned views


@pytest.mark.parametrize('config', ['adam_wd1e-4', 'adamw_wd0.01', 'sgd_nesterov_wd'])
def test_steps_against_float64_above_the_launch_caps(inputs_above, config):
    """the same rule on _sizes_above(); every tensor's counter is read after every step"""
    _steps_against_float64(inputs_above, config, 'steps_above', all_steps=True)


def _norm64(inputs, step):
    g = inputs['grads'][step].astype(np.float64)
    return math.sqrt(float(np.sum(g * g)))


def _fused_in_clip(inputs, where, key):
    """optimizer.clip_grad_norm: the norm against float64 within 2 ulp (the sum is in double: what is
    left is its rounding to float32 and one sqrt), the update against the float64 formula with the
    float64 clip coefficient, .grad left as it was; torch's clip_grad_norm_ + step is the stock side."""
    name, kw = CONFIGS['adam_wd1e-4']
    norms = [_norm64(inputs, s) for s in range(STEPS)]
    max_norm = min(norms) * 0.37 if where == 'below' else max(norms) * 2.0
    max_norm = float(np.float32(max_norm))       # (exact in float32: no rounding on its way into the kernel)
    coef = [min(1.0, max_norm / (n + 1e-6)) for n in norms]
    assert all(c < 1 for c in coef) if where == 'below' else all(c == 1 for c in coef)
    ref = _reference(inputs, name, kw, coef=coef)
    seen = []

    def stock_clip(opt, params):
        torch.nn.utils.clip_grad_norm_(params, max_norm)

    def fused_clip(opt, params):
        opt.clip_grad_norm = max_norm
        if opt.last_grad_norm is not None:
            seen.append(opt.last_grad_norm.clone())

    stock = _run(inputs, name, kw, fused=False, before_step=stock_clip)
    fused = _run(inputs, name, kw, fused=True, before_step=fused_clip)
    first = list(seen)
    del seen[:]
    again = _run(inputs, name, kw, fused=True, before_step=fused_clip)
    figures = {}
    for step in range(STEPS):
        es, ef = _ulps(stock[step][0], ref[step][0]), _ulps(fused[step][0], ref[step][0])
        figures[f'step {step + 1} p'] = (es, ef)
        print(f'clip {where} step {step + 1} p stock {es:.4f} ulp   fused {ef:.4f} ulp')
        assert np.array_equal(fused[step][0], again[step][0])
    # last_grad_norm of steps 1 .. STEPS - 1 (read at the start of the following step)
    for step, (a, b) in enumerate(zip(first, seen)):
        e = _ulps(np.array([float(a)]), np.array([norms[step]]))
        figures[f'step {step + 1} norm'] = (0.0, e)
        print(f'clip {where} step {step + 1} norm {float(a):.9g} vs {norms[step]:.12g}: {e:.3f} ulp')
        assert e <= 2.0, (step, float(a), norms[step])
        assert torch.equal(a, b)
    _record(f'{key}[{where}]', figures)
    for step in range(STEPS):
        es, ef = figures[f'step {step + 1} p']
        assert ef <= 2 * es + 1, (step, es, ef)


@pytest.mark.parametrize('where', ['below', 'above'])
def test_fused_in_clip(inputs, where):
    _fused_in_clip(inputs, where, 'clip')


def test_fused_in_clip_above_the_launch_caps(inputs_above):
    """grad_norm_kernel in its third trip, the clipped step in its second"""
    _fused_in_clip(inputs_above, 'below', 'clip_above')


def test_fused_in_clip_leaves_grad_alone(inputs):
    params = _params(inputs)
    opt = O.FusedSGD(params, lr=0.01)
    opt.clip_grad_norm = 0.5
    _set_grads(params, inputs, 0)
    before = [p.grad.clone() for p in params]
    opt.step()
    assert all(torch.equal(a, p.grad) for a, p in zip(before, params))
    e = _ulps(np.array([float(opt.last_grad_norm)]), np.array([_norm64(inputs, 0)]))
    assert e <= 2.0, e


def _standalone_clip_grad_norm(inputs, where, key):
    """clip_grad_norm_ against torch's own function.  Ours: the float32 norm within 2 ulp of float64
    (as above); coef = max_norm / (norm + 1e-6) adds two float32 roundings (0.5 ulp each) and the
    product one more: 2 + 1.5 = 3.5 ulp relative, up to twice that where a value sits just above a
    power of two and the reference just below: 7 ulp.  torch's own norm is a float32 reduction of
    per-tensor float32 norms; its measured error E_t replaces the 2."""
    norm = _norm64(inputs, 0)
    max_norm = float(np.float32(norm * (0.37 if where == 'below' else 2.0)))      # (exact in float32)
    coef = min(1.0, max_norm / (norm + 1e-6))
    want = inputs['grads'][0].astype(np.float64) * coef
    results = []
    for fn in (torch.nn.utils.clip_grad_norm_, O.clip_grad_norm_, O.clip_grad_norm_):
        params = _params(inputs)
        _set_grads(params, inputs, 0)
        versions = [p.grad._version for p in params]
        ret = fn(params, max_norm)
        assert ret.shape == () and ret.dtype == torch.float32 and ret.is_cuda
        if fn is O.clip_grad_norm_:
            assert all(p.grad._version > v for p, v in zip(params, versions) if p.numel())
        results.append((float(ret), _flat([p.grad for p in params])))
    (tn, tg), (on, og), (on2, og2) = results
    et, eo = _ulps(np.array([tn]), np.array([norm])), _ulps(np.array([on]), np.array([norm]))
    gt, go = _ulps(tg, want), _ulps(og, want)
    print(f'clip_grad_norm_ {where}: norm torch {et:.3f} ulp, ours {eo:.3f} ulp; grads torch {gt:.3f}, ours {go:.3f}')
    _record(f'{key}[{where}]', {'norm': (et, eo), 'grads': (gt, go)})
    assert eo <= 2.0
    assert on == on2 and np.array_equal(og, og2)                      # two runs: the same bits
    if where == 'above':
        assert np.array_equal(og, inputs['grads'][0]) and np.array_equal(og, tg)
    else:
        assert go <= 7.0, go
        # against torch's own result: both sides' distance to the float64 value
        assert _ulps(np.array([on]), np.array([tn], dtype=np.float64)) <= 2.0 + et + 1.0
        assert _ulps(og, tg.astype(np.float64)) <= 7.0 + 2 * (et + 1.5) + 1.0
    # a norm_type other than 2 goes to torch
    params = _params(inputs)
    _set_grads(params, inputs, 0)
    a = O.clip_grad_norm_(params, max_norm, norm_type=1.0)
    q = _params(inputs)
    _set_grads(q, inputs, 0)
    b = torch.nn.utils.clip_grad_norm_(q, max_norm, norm_type=1.0)
    assert torch.equal(a, b) and all(torch.equal(x.grad, y.grad) for x, y in zip(params, q))


@pytest.mark.parametrize('where', ['below', 'above'])
def test_standalone_clip_grad_norm(inputs, where):
    _standalone_clip_grad_norm(inputs, where, 'clip_grad_norm_')


def test_standalone_clip_grad_norm_above_the_launch_caps(inputs_above):
    """grad_norm_kernel in its third trip, scale_grads_kernel in its second"""
    _standalone_clip_grad_norm(inputs_above, 'below', 'clip_grad_norm_above')


def test_states_sharing_a_misaligned_start(inputs):
    """parameter, gradient and both states at the same odd element offset: the walk's scalar head, a
    16-byte body and a scalar tail (fresh states are aligned, which sends a misaligned parameter down
    the all-scalar path instead)"""
    n = O.chunk_elems() + 7
    rng = np.random.default_rng(8)
    vals = [rng.standard_normal(n).astype(np.float32) for _ in range(4)]
    vals[3] = np.abs(vals[3])
    kw = dict(lr=1e-2, weight_decay=1e-4)

    def run(cls, off):
        bufs = [torch.zeros(n + 8, device=DEV) for _ in range(4)]
        p, g, m, v = [b[off:off + n] for b in bufs]
        for t, a in zip((p, g, m, v), vals):
            t.copy_(torch.from_numpy(a))
        p.requires_grad_(True)
        opt = cls([p], **kw)
        opt.state[p] = dict(step=torch.full((), 4.0, device=DEV) if off else torch.tensor(4.0), exp_avg=m,
                            exp_avg_sq=v)
        p.grad = g
        opt.step()
        if off:
            assert opt._sg_plan is not None and m.data_ptr() % 16 == 4 * off
        return [t.detach().cpu().numpy() for t in (p, m, v)], float(opt.state[p]['step'])

    want = _adam64(*[a.astype(np.float64) for a in (vals[0], vals[2], vals[3], vals[1])], 5, **kw)
    stock, _ = run(torch.optim.Adam, 0)
    for off in (1, 2, 3):
        fused, step = run(O.FusedAdam, off)
        assert step == 5.0
        for what, w, s_, f_ in zip(('p', 'exp_avg', 'exp_avg_sq'), want, stock, fused):
            es, ef = _ulps(s_, w), _ulps(f_, w)
            print(f'misaligned by {off}: {what:<12s} stock {es:.4f} ulp   fused {ef:.4f} ulp')
            assert ef <= 2 * es + 1, (off, what, es, ef)


# ---- AMP ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('config', ['adam_wd1e-4', 'sgd_nesterov_wd'])
def test_grad_scale_power_of_two_is_exact(inputs, config):
    name, kw = CONFIGS[config]
    plain = _run(inputs, name, kw, fused=True)

    def scaled(opt, params):
        for p in params:
            p.grad.mul_(1024.0)
        opt.grad_scale = torch.full((), 1024.0, device=DEV)
        opt.found_inf = torch.zeros((), device=DEV)
        opt.clip_grad_norm = None

    amp = _run(inputs, name, kw, fused=True, before_step=scaled)
    for step in range(STEPS):
        assert np.array_equal(plain[step][0], amp[step][0])
        for a, b in zip(plain[step][1], amp[step][1]):
            assert (a is None and b is None) or np.array_equal(a, b)


def _found_inf_writes_nothing(inputs, config):
    name, kw = CONFIGS[config]
    params = _params(inputs)
    opt = O.FUSED_CLASSES[name](params, **kw)
    opt.clip_grad_norm = 1.0
    _set_grads(params, inputs, 0)
    opt.step()                                   # states exist, counters at 1

    def snapshot():
        out = [p.detach().clone() for p in params]
        for p in params:
            out += [v.clone() for v in opt.state[p].values() if torch.is_tensor(v)]
        return out

    before = snapshot()
    for bad in (float('inf'), float('nan')):
        _set_grads(params, inputs, 1, scale=1024.0)
        params[-1].grad[2] = bad                 # one element of a tensor of the last chunk
        opt.grad_scale = torch.full((), 1024.0, device=DEV)
        opt.found_inf = torch.ones((), device=DEV)
        opt.step()
        after = snapshot()
        assert len(before) == len(after) and all(
            torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, after))
    # and the step after it is a normal second step
    del opt.grad_scale, opt.found_inf
    _set_grads(params, inputs, 1)
    opt.step()
    assert float(opt.state[params[0]]['step']) == 2.0
    assert not torch.equal(before[0], params[0].detach())


@pytest.mark.parametrize('config', ['adam_wd1e-4', 'sgd_nesterov_wd'])
def test_found_inf_writes_nothing(inputs, config):
    _found_inf_writes_nothing(inputs, config)


@pytest.mark.parametrize('config', ['adam_wd1e-4', 'sgd_nesterov_wd'])
def test_found_inf_writes_nothing_above_the_launch_caps(inputs_above, config):
    _found_inf_writes_nothing(inputs_above, config)


def test_grad_scaler_loop_matches_stock():
    """scaler.scale(loss).backward(); scaler.step(opt); scaler.update() for 2 steps on a 3-tensor toy,
    the first overflowing: the same scale afterwards, and parameters within the tolerance of the step
    test against the float64 formula of the one step that was taken."""
    torch.manual_seed(3)
    shapes = [(33, ), (7, 9), (130, )]
    init = [torch.randn(s, device=DEV) for s in shapes]
    xs = [[torch.randn(s, device=DEV) for s in shapes] for _ in range(2)]
    xs[0][1][3, 4] = 3e36                        # times the scale of 65536: inf in float32
    kw = dict(lr=1e-2, weight_decay=1e-4)

    def loop(cls):
        params = [t.clone().requires_grad_(True) for t in init]
        opt = cls(params, **kw)
        scaler = torch.amp.GradScaler('cuda')
        for x in xs:
            loss = sum((p * a).sum() for p, a in zip(params, x))
            opt.zero_grad()
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
        return params, float(scaler.get_scale()), opt

    sp, s_scale, _ = loop(torch.optim.Adam)
    fp, f_scale, opt = loop(O.FusedAdam)
    assert s_scale == f_scale == 32768.0
    assert all(float(opt.state[p]['step']) == 1.0 for p in fp)       # the overflowing step was skipped
    p64 = np.concatenate([t.cpu().numpy().reshape(-1) for t in init]).astype(np.float64)
    g64 = np.concatenate([t.cpu().numpy().reshape(-1) for t in xs[1]]).astype(np.float64)
    want, _, _ = _adam64(p64, np.zeros_like(p64), np.zeros_like(p64), g64, 1, **kw)
    es, ef = _ulps(_flat(sp), want), _ulps(_flat(fp), want)
    print(f'GradScaler loop: stock {es:.4f} ulp   fused {ef:.4f} ulp')
    _record('grad_scaler_loop', {'p': (es, ef)})
    assert ef <= 2 * es + 1, (es, ef)


# ---- the cache trap -----------------------------------------------------------------------------
def test_step_invalidates_packed_weight_caches():
    import softgroup_amd.spconv.pytorch as spconv
    from softgroup_amd.spconv import core
    rng = np.random.default_rng(5)
    shape = [16, 16, 16]
    vox = np.unique(rng.integers(0, 16, (260, 3)), axis=0)[:200]
    idx = np.concatenate([np.zeros((len(vox), 1), np.int64), vox], 1).astype(np.int32)
    feats = torch.from_numpy(rng.standard_normal((len(idx), 16)).astype(np.float32)).to(DEV)
    ti = torch.from_numpy(idx).to(DEV)
    torch.manual_seed(0)
    conv = spconv.SubMConv3d(16, 16, kernel_size=3, padding=1, bias=False, indice_key='k').to(DEV)
    opt = O.FusedAdam(conv.parameters(), lr=0.05)

    def forward():
        return conv(spconv.SparseConvTensor(feats, ti, shape, 1)).features

    out0 = forward()
    out0.square().sum().backward()
    versions = [p._version for p in conv.parameters()]
    with torch.no_grad():
        before = forward().clone()
    opt.step()
    assert opt._sg_plan is not None              # (the fused path, not the torch step)
    assert all(p._version > v for p, v in zip(conv.parameters(), versions))
    with torch.no_grad():
        after = forward().clone()
        core.invalidate_caches()
        fresh = forward().clone()
    assert torch.equal(after, fresh)
    assert not torch.equal(after, before)


# ---- model level --------------------------------------------------------------------------------
def test_model_two_steps_fused_vs_stock():
    xyz, rgb, inst = synthetic.scene_s2(seed=21, n=20000, room_scale=0.45)
    batch = synthetic.make_batch(xyz, rgb, instance_labels=inst)
    model = synthetic.build_model(synthetic.SCANNET_MODEL_CFG, seed=0)
    model.train()
    start = copy.deepcopy(model.state_dict())
    kw = dict(lr=1e-3)

    def run(fused):
        model.load_state_dict(start)
        opt = O.build_optimizer(model, dict(type='Adam', **kw), fused=fused)
        assert isinstance(opt, O.FusedAdam) == fused
        params = [p for g in opt.param_groups for p in g['params']]
        info = {}
        for step in range(2):
            torch.manual_seed(11 + step)
            loss, _ = model(batch, return_loss=True)
            opt.zero_grad()
            loss.backward()
            if step == 0:
                live = [p for p in params if p.grad is not None]
                info['p0'] = _flat(live).astype(np.float64)
                info['g'] = _flat([p.grad for p in live]).astype(np.float64)
                info['live'] = live
            opt.step()
            if step == 0:
                info['p1'] = _flat(info['live'])
            info[f'loss{step + 1}'] = float(loss)
        return info

    f, s = run(True), run(False)
    assert len(f['live']) > 10
    # step 1: each side against the float64 formula on its own float32 gradients
    errs = []
    for r in (s, f):
        want, _, _ = _adam64(r['p0'], np.zeros_like(r['p0']), np.zeros_like(r['p0']), r['g'], 1, **kw)
        errs.append(_ulps(r['p1'], want))
    print(f'model step 1: stock {errs[0]:.4f} ulp   fused {errs[1]:.4f} ulp; '
          f'loss 1 {s["loss1"]:.7f} / {f["loss1"]:.7f}   loss 2 {s["loss2"]:.7f} / {f["loss2"]:.7f}')
    _record('model', {'step 1 p': tuple(errs)})
    assert errs[1] <= 2 * errs[0] + 1, errs
    assert abs(f['loss2'] - s['loss2']) <= 1e-4 * abs(s['loss2']), (f['loss2'], s['loss2'])
    # every parameter with a gradient moved (a zero gradient moves nothing under Adam: m = 0)
    at = 0
    for p in f['live']:
        n = p.numel()
        g = f['g'][at:at + n]
        if np.any(g != 0):
            assert np.any(f['p1'][at:at + n].astype(np.float64) != f['p0'][at:at + n])
        at += n


# ---- fallback on the device ---------------------------------------------------------------------
@pytest.mark.parametrize('why', ['bf16', 'amsgrad'])
def test_device_fallback_is_the_parent_step(why):
    torch.manual_seed(9)
    init = [torch.randn(300, device=DEV), torch.randn(17, 5, device=DEV), torch.randn(64, device=DEV)]
    if why == 'bf16':
        init[1] = init[1].bfloat16()
    kw = dict(lr=1e-2, amsgrad=why == 'amsgrad')
    grads = [[torch.randn_like(t) for t in init] for _ in range(2)]

    def loop(cls):
        params = [t.clone().requires_grad_(True) for t in init] + [torch.ones(8, device=DEV, requires_grad=True)]
        opt = cls(params, **kw)
        for gs in grads:
            for p, g in zip(params, gs):          # (the last parameter never has a gradient)
                p.grad = g.clone()
            opt.step()
        return params, opt

    sp, _ = loop(torch.optim.Adam)
    fp, opt = loop(O.FusedAdam)
    assert all(torch.equal(a, b) for a, b in zip(sp, fp))
    assert torch.equal(fp[-1].detach(), torch.ones(8, device=DEV)) and fp[-1] not in opt.state
    assert opt._sg_plan is None                  # (nothing was built for the kernels)


def test_grad_none_untouched_on_the_fused_path():
    torch.manual_seed(2)
    a = torch.randn(100, device=DEV, requires_grad=True)
    b = torch.randn(50, device=DEV, requires_grad=True)
    keep = b.detach().clone()
    opt = O.FusedAdamW([a, b], lr=0.1)
    a.grad = torch.randn_like(a)
    opt.step()
    assert torch.equal(b.detach(), keep) and b not in opt.state and float(opt.state[a]['step']) == 1.0
    # and a state-dict round trip through the stock class keeps going
    b.grad = torch.randn_like(b)
    opt.step()
    stock = torch.optim.AdamW([a, b], lr=0.1)
    stock.load_state_dict(opt.state_dict())
    back = O.FusedAdamW([a, b], lr=0.1)
    back.load_state_dict(stock.state_dict())
    st = back.state[a]['step']
    assert st.is_cuda and st.dtype == torch.float32 and float(st) == 2.0 and float(back.state[b]['step']) == 1.0
    a.grad, b.grad = torch.randn_like(a), torch.randn_like(b)
    back.step()
    assert float(back.state[a]['step']) == 3.0
