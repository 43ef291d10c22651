"""Fused loss kernels (csrc/losses.hip) through ctypes and the C ABI against the formulas of the reference's
point_wise_loss / instance_loss (softgroup/model/softgroup.py:152-255) evaluated by torch in float64 on the CPU.

Bounds: loss values within LOSS_RTOL = 1e-4 relative (the project's bound, tests/test_train_gpu.py), counts
exact, gradients within 1e-4 of each tensor's largest reference entry, NaN positions equal; labels equal.  Every
kernel runs twice on the same inputs and must return the same bits."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from softgroup_amd import _lib as L
from softgroup_amd import ops
from softgroup_amd.model import SoftGroup
from softgroup_amd.model.softgroup import _assign_proposals
from test_losses_cpu import _reference_labels
from test_train_gpu import GT, LOSS_RTOL, _train_case

pytestmark = pytest.mark.gpu
DEV = 'cuda'
IGN = -100


# ------------------------------------------------------------------------------------------------ helpers
def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _loss_close(got, want, what):
    got, want = float(got), float(want)
    print(what, got, want)
    if np.isnan(want):
        assert np.isnan(got), (what, got, want)
    else:
        assert abs(got - want) <= LOSS_RTOL * max(abs(want), 1e-3), (what, got, want)


def _grad_close(got, want, what):
    """1e-4 of the tensor's largest reference entry; NaN positions equal"""
    got, want = got.double().cpu(), want.double()
    assert got.shape == want.shape, what
    if want.numel() == 0:
        return
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), what
    scale = float(want[~nan].abs().max()) if (~nan).any() else 0.0
    err = float((got - want)[~nan].abs().max()) if (~nan).any() else 0.0
    print(what, 'max |d|', err, 'scale', scale)
    assert err <= 1e-4 * scale, (what, err, scale)


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=DEV)


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


# ------------------------------------------------------------------------------------------------ point-wise
def _pw_case(n, c, seed, weighted, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(n, c, generator=g) * scale
    y = torch.randint(0, c, (n, ), generator=g)
    y[::7] = IGN
    o, ol = torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g)
    inst = torch.randint(0, 4, (n, ), generator=g)
    inst[1::3] = IGN
    w = torch.rand(c, generator=g) + 0.1 if weighted else None
    return dict(s=s, y=y, w=w, o=o, ol=ol, inst=inst)


def _pw_run(case, gs=0.7, go=1.3, want_s=True, want_o=True):
    lib = L.lib()
    n, c = case['s'].shape
    s, y, w, o, ol, inst = (_dev(case[k]) for k in ('s', 'y', 'w', 'o', 'ol', 'inst'))
    out = torch.full((6, ), 7.0, device=DEV)
    ws = _ws(lib.sg_loss_reduce_workspace_bytes())
    L.check(lib.sg_pointwise_loss_fwd(L.ptr(s), L.ptr(y), L.ptr(w), IGN, L.ptr(o), L.ptr(ol), L.ptr(inst), n, c,
                                      L.ptr(out), L.ptr(ws), ws.numel(), L.stream()), 'fwd')
    d_s = torch.full((n, c), 7.0, device=DEV) if want_s else None
    d_o = torch.full((n, 3), 7.0, device=DEV) if want_o else None
    g_s = None if gs is None else torch.tensor(gs, device=DEV)
    g_o = None if go is None else torch.tensor(go, device=DEV)
    L.check(lib.sg_pointwise_loss_bwd(L.ptr(s), L.ptr(y), L.ptr(w), IGN, L.ptr(o), L.ptr(ol), L.ptr(inst), n, c,
                                      L.ptr(out), L.ptr(g_s), L.ptr(g_o), L.ptr(d_s), L.ptr(d_o), L.stream()), 'bwd')
    torch.cuda.synchronize()
    return out, d_s, d_o


def _pw_ref(case, gs=0.7, go=1.3):
    """softgroup.py:159-169 in float64"""
    s = case['s'].double().requires_grad_(True)
    o = case['o'].double().requires_grad_(True)
    w = None if case['w'] is None else case['w'].double()
    sem = F.cross_entropy(s, case['y'], weight=w, ignore_index=IGN) if s.numel() else s.sum() / 0
    pos = case['inst'] != IGN
    if pos.sum() == 0:
        off = 0 * o.sum()
    else:
        off = F.l1_loss(o[pos], case['ol'].double()[pos], reduction='sum') / pos.sum()
    d_s, = torch.autograd.grad(gs * sem, s)
    d_o, = torch.autograd.grad(go * off, o)
    valid = (case['y'] != IGN)
    wsum = float(valid.sum()) if w is None else float(w[case['y'][valid]].sum())
    return dict(sem=sem.detach(), off=off.detach(), d_s=d_s, d_o=d_o, wsum=wsum, npos=int(pos.sum()))


def _pw_check(case, what):
    out, d_s, d_o = _pw_run(case)
    ref = _pw_ref(case)
    _loss_close(out[4], ref['sem'], what + ' semantic_loss')
    _loss_close(out[5], ref['off'], what + ' offset_loss')
    _loss_close(out[1], ref['wsum'], what + ' sum w')
    assert float(out[3]) == ref['npos'], what
    if ref['wsum'] > 0:
        _loss_close(out[0], float(ref['sem']) * ref['wsum'], what + ' sum w nll')
    _grad_close(d_s, ref['d_s'], what + ' d_scores')
    _grad_close(d_o, ref['d_o'], what + ' d_offsets')
    again = _pw_run(case)
    assert _same_bits((out, d_s, d_o), again), what + ': two runs differ'
    return out, d_s, d_o


@pytest.mark.parametrize('c', [1, 2, 13, 20, 64])
def test_point_wise_loss_shapes(c):
    for n in (0, 1, 63, 64, 65, 257, 5000):
        for weighted in (False, True):
            _pw_check(_pw_case(n, c, 100 * c + n, weighted), f'n={n} c={c} w={weighted}')


@pytest.mark.parametrize('n,c', [(257, 13), (5000, 20)])
def test_point_wise_loss_edge_cases(n, c):
    # all labels ignored: NaN loss (F.cross_entropy), zero gradient
    case = _pw_case(n, c, 1, True)
    case['y'][:] = IGN
    out, d_s, _ = _pw_check(case, 'all ignored')
    assert torch.isnan(out[4]) and float(d_s.abs().max()) == 0.0
    # no instance point: 0 and a zero gradient (softgroup.py:164-165)
    case = _pw_case(n, c, 2, False)
    case['inst'][:] = IGN
    out, _, d_o = _pw_check(case, 'no instance point')
    assert float(out[5]) == 0.0 and float(out[3]) == 0.0 and float(d_o.abs().max()) == 0.0
    # scores x 50: only a max-subtracted log-sum-exp survives
    out, _, _ = _pw_check(_pw_case(n, c, 3, True, scale=50.0), 'scores x 50')
    assert torch.isfinite(out[4])
    # rows with delta == 0 exactly: sign(0) = 0
    case = _pw_case(n, c, 4, False)
    case['ol'][::2] = case['o'][::2]
    case['ol'][1::4, 1] = case['o'][1::4, 1]
    _, _, d_o = _pw_check(case, 'delta == 0')
    assert float(d_o[::2].abs().max()) == 0.0
    # labels outside [0, c) that are not ignore_label == those rows ignored
    case = _pw_case(n, c, 5, True)
    bad = case['y'].clone()
    bad[3::11] = c
    bad[5::13] = -1
    bad[2] = 2 ** 40
    as_ignored = dict(case, y=torch.where((bad < 0) | (bad >= c), torch.full_like(bad, IGN), bad))
    got = _pw_run(dict(case, y=bad))
    want = _pw_check(as_ignored, 'out-of-range labels as ignored')
    assert _same_bits(got, want)


def test_point_wise_loss_each_gradient_alone():
    case = _pw_case(257, 13, 6, True)
    out, d_s, d_o = _pw_run(case)
    o1, s1, none = _pw_run(case, want_o=False)
    assert none is None and _same_bits((out, d_s), (o1, s1))
    o2, none, only_o = _pw_run(case, want_s=False)
    assert none is None and _same_bits((out, d_o), (o2, only_o))
    # a missing upstream gradient is a zero one
    _, z_s, z_o = _pw_run(case, gs=None, go=1.3)
    assert float(z_s.abs().max()) == 0.0 and _same_bits((z_o, ), (d_o, ))
    _, z_s, z_o = _pw_run(case, gs=0.7, go=None)
    assert float(z_o.abs().max()) == 0.0 and _same_bits((z_s, ), (d_s, ))


# ------------------------------------------------------------------------------------------------ assignment
def _assign(ious, cls, thr, mlq, min_pos, background):
    lib = L.lib()
    n_prop, n_gt = ious.shape
    i, c = _dev(ious), _dev(cls)
    labels = torch.full((n_prop, ), -7, dtype=torch.int64, device=DEV)
    ws = _ws(lib.sg_assign_proposals_workspace_bytes(n_prop))
    L.check(lib.sg_assign_proposals(L.ptr(i), L.ptr(c), IGN, thr, int(mlq), min_pos, background, n_prop, n_gt,
                                    L.ptr(labels), L.ptr(ws), ws.numel(), L.stream()), 'sg_assign_proposals')
    return labels.cpu()


def _assign_check(ious, cls, what):
    for mlq in (False, True):
        for min_pos in (0.0, 0.1):
            got = _assign(ious, cls, 0.5, mlq, min_pos, 18)
            assert torch.equal(got, _assign_proposals(ious, cls, cls != IGN, 0.5, mlq, min_pos, 18)), (what, mlq, min_pos)
            assert torch.equal(got, _reference_labels(ious, cls, 0.5, mlq, min_pos, 18)), (what, mlq, min_pos)
            assert torch.equal(got, _assign(ious, cls, 0.5, mlq, min_pos, 18)), (what, 'two runs differ')


def test_assignment_generator_of_the_cpu_test():
    g = torch.Generator().manual_seed(1)
    checked = 0
    for trial in range(400):
        n_prop = int(torch.randint(1, 14, (1, ), generator=g))
        n_gt = int(torch.randint(1, 10, (1, ), generator=g))
        ious = torch.rand(n_prop, n_gt, generator=g)
        ious[torch.rand(n_prop, n_gt, generator=g) < 0.35] = 0
        if trial % 5 == 0:
            ious[:, 0] = ious[:, -1]
        cls = torch.randint(0, 6, (n_gt, ), generator=g)
        cls[torch.rand(n_gt, generator=g) < 0.3] = IGN
        if int((cls != IGN).sum()) == 0:
            continue
        _assign_check(ious, cls, trial)
        checked += 4
    assert checked > 1000


@pytest.mark.parametrize('n_prop', [1, 64, 65, 300])
def test_assignment_shapes(n_prop):
    for n_gt in (1, 64, 130):
        g = torch.Generator().manual_seed(n_prop * 1000 + n_gt)
        ious = (torch.rand(n_prop, n_gt, generator=g) * 8).round() / 8        # many exact ties
        ious[torch.rand(n_prop, n_gt, generator=g) < 0.35] = 0
        if n_gt > 1:
            ious[:, 0] = ious[:, -1]
        cls = torch.randint(0, 18, (n_gt, ), generator=g)
        cls[torch.rand(n_gt, generator=g) < 0.3] = IGN
        cls[n_gt // 2] = 3
        _assign_check(ious, cls, (n_prop, n_gt))


# ------------------------------------------------------------------------------------------------ proposal + mask
SPECIAL = (20.0, -20.0, 40.0, -40.0, 100.0, -100.0)


def _inst_case(n_prop, k1, m, seed, all_background=False):
    g = torch.Generator().manual_seed(seed)
    n_gt = 130 if n_prop % 2 else 7
    labels = torch.randint(0, k1, (n_prop, ), generator=g)
    if all_background:
        labels[:] = k1 - 1
    bidx = torch.randint(0, n_prop, (m, ), generator=g, dtype=torch.int32)
    ms = 3 * torch.randn(m, k1, generator=g)
    # every 5th point: a saturating logit in its class column, against every mask label in turn
    i = torch.arange(0, m, 5)
    col = labels[bidx[i].long()]
    ms[i, col] = torch.tensor(SPECIAL)[(i // 5) % 6]
    ml = torch.randint(-1, 2, (m, ), generator=g).float()
    ml[i] = ((i // 30) % 3 - 1).float()
    cls = torch.randint(0, k1 - 1, (n_gt, ), generator=g)
    cls[torch.rand(n_gt, generator=g) < 0.3] = IGN
    cls[n_gt // 2] = 0
    return dict(cs=2 * torch.randn(n_prop, k1, generator=g), io=torch.randn(n_prop, k1, generator=g), labels=labels,
                ious=torch.rand(n_prop, n_gt, generator=g), cls=cls, ms=ms, bidx=bidx, ml=ml)


def _inst_run(case, g=(1.0, 2.0, 3.0)):
    lib = L.lib()
    n_prop, k1 = case['cs'].shape
    m = case['ms'].shape[0]
    n_gt = case['cls'].numel()
    cs, io, labels, ious, cls, ms, bidx, ml = (_dev(case[k]) for k in ('cs', 'io', 'labels', 'ious', 'cls', 'ms', 'bidx', 'ml'))
    ws = _ws(lib.sg_loss_reduce_workspace_bytes())
    mout, pout = torch.full((6, ), 7.0, device=DEV), torch.full((6, ), 7.0, device=DEV)
    sig = torch.full((m, ), 7.0, device=DEV)
    L.check(lib.sg_mask_loss_fwd(L.ptr(ms), L.ptr(bidx), L.ptr(labels), L.ptr(ml), m, n_prop, k1, L.ptr(sig),
                                 L.ptr(mout), L.ptr(ws), ws.numel(), L.stream()), 'sg_mask_loss_fwd')
    gt_iou = torch.full((n_prop, ), 7.0, device=DEV)
    L.check(lib.sg_proposal_loss_fwd(L.ptr(cs), L.ptr(io), L.ptr(labels), L.ptr(ious), L.ptr(cls), IGN, n_prop, n_gt,
                                     k1, L.ptr(gt_iou), L.ptr(pout), L.ptr(ws), ws.numel(), L.stream()),
            'sg_proposal_loss_fwd')
    gc, gm, gi = (torch.tensor(v, device=DEV) for v in g)
    d_ms, d_cs, d_io = (torch.full(t.shape, 7.0, device=DEV) for t in (ms, cs, io))
    L.check(lib.sg_mask_loss_bwd(L.ptr(ms), L.ptr(bidx), L.ptr(labels), L.ptr(ml), L.ptr(mout), L.ptr(gm), m, n_prop,
                                 k1, L.ptr(d_ms), L.stream()), 'sg_mask_loss_bwd')
    L.check(lib.sg_proposal_loss_bwd(L.ptr(cs), L.ptr(io), L.ptr(labels), L.ptr(gt_iou), L.ptr(pout), L.ptr(gc),
                                     L.ptr(gi), n_prop, k1, L.ptr(d_cs), L.ptr(d_io), L.stream()),
            'sg_proposal_loss_bwd')
    torch.cuda.synchronize()
    return mout, pout, sig, gt_iou, d_ms, d_cs, d_io


def _inst_ref(case, g=(1.0, 2.0, 3.0)):
    """softgroup.py:223-255 in float64"""
    n_prop, k1 = case['cs'].shape
    m = case['ms'].shape[0]
    cs, io, ms = (case[k].double().requires_grad_(True) for k in ('cs', 'io', 'ms'))
    labels = case['labels']
    cls_loss = F.cross_entropy(cs, labels)
    sig = ms.sigmoid()[torch.arange(m), labels[case['bidx'].long()]]
    ml = case['ml'].double()
    w = (ml != -1).double()
    y = torch.where(ml == -1, torch.full_like(ml, 0.5), ml)
    mask_sum = F.binary_cross_entropy(sig, y, weight=w, reduction='sum')
    mask_loss = mask_sum / (w.sum() + 1)
    gt = case['ious'].double()[:, case['cls'] != IGN].max(1)[0]
    wi = (labels < k1 - 1).double()
    iou_loss = (F.mse_loss(io[torch.arange(n_prop), labels], gt, reduction='none') * wi).sum() / (wi.sum() + 1)
    d_cs, d_ms, d_io = torch.autograd.grad(g[0] * cls_loss + g[1] * mask_loss + g[2] * iou_loss, (cs, ms, io),
                                           allow_unused=True)
    return dict(cls_loss=cls_loss.detach(), mask_loss=mask_loss.detach(), iou_loss=iou_loss.detach(),
                mask_sum=mask_sum.detach(), w=float(w.sum()), num_pos=float(wi.sum()), num_neg=float((1 - wi).sum()),
                gt=gt, d_cs=d_cs, d_ms=d_ms if d_ms is not None else torch.zeros_like(ms), d_io=d_io)


def _inst_check(case, what):
    got = _inst_run(case)
    mout, pout, sig, gt_iou, d_ms, d_cs, d_io = got
    ref = _inst_ref(case)
    m, k1 = case['ms'].shape
    _loss_close(pout[4], ref['cls_loss'], what + ' cls_loss')
    _loss_close(pout[5], ref['iou_loss'], what + ' iou_score_loss')
    _loss_close(mout[4], ref['mask_loss'], what + ' mask_loss')
    _loss_close(mout[0], ref['mask_sum'], what + ' bce sum')
    assert float(mout[1]) == ref['w'] and float(pout[2]) == ref['num_pos'] and float(pout[3]) == ref['num_neg'], what
    assert float((gt_iou.cpu().double() - ref['gt']).abs().max()) == 0.0, what
    want_sig = torch.sigmoid(case['ms'])[torch.arange(m), case['labels'][case['bidx'].long()]]
    if m:
        assert float((sig.cpu() - want_sig).abs().max()) <= 1e-6, what
    _grad_close(d_cs, ref['d_cs'], what + ' d_cls_scores')
    _grad_close(d_io, ref['d_io'], what + ' d_iou_scores')
    _grad_close(d_ms, ref['d_ms'], what + ' d_mask_scores')
    # one entry per row at most: every other column is exactly zero
    if m:
        other = torch.ones(m, k1, dtype=torch.bool)
        other[torch.arange(m), case['labels'][case['bidx'].long()]] = False
        assert float(d_ms.cpu()[other].abs().max()) == 0.0, what
    other = torch.ones_like(case['io'], dtype=torch.bool)
    other[torch.arange(case['io'].shape[0]), case['labels']] = False
    assert float(d_io.cpu()[other].abs().max()) == 0.0, what
    assert _same_bits(got, _inst_run(case)), what + ': two runs differ'
    return got, ref


@pytest.mark.parametrize('n_prop', [1, 3, 65, 300])
@pytest.mark.parametrize('k1', [2, 19])
def test_proposal_and_mask_losses(n_prop, k1):
    for m in (0, 1, 255, 256, 257, 20000):
        _inst_check(_inst_case(n_prop, k1, m, 7 * n_prop + k1 + m), f'P={n_prop} K+1={k1} M={m}')


def test_all_proposals_background():
    """sum w = 0: both weighted losses are sums over '+ 1' (softgroup.py:237, 249)"""
    (mout, pout, *_), ref = _inst_check(_inst_case(65, 19, 257, 11, all_background=True), 'all background')
    assert float(pout[2]) == 0.0 and float(pout[3]) == 65.0 and float(pout[5]) == 0.0
    case = _inst_case(65, 19, 257, 12)
    case['ml'][:] = -1.0
    (mout, *_), _ = _inst_check(case, 'all mask labels ignored')
    assert float(mout[1]) == 0.0 and float(mout[4]) == 0.0


def test_saturated_logits_follow_the_formulas():
    """the -100 clamp of binary_cross_entropy and the 1e-12 floor of its backward, at the logits that reach them"""
    n = len(SPECIAL) * 3
    case = _inst_case(1, 2, n, 13)
    case['labels'][:] = 0
    case['ms'][:, 0] = torch.tensor(SPECIAL).repeat_interleave(3)
    case['ml'] = torch.tensor([-1.0, 0.0, 1.0]).repeat(len(SPECIAL))
    (mout, _, _, _, d_ms, _, _), ref = _inst_check(case, 'saturated')
    d = d_ms.cpu()[:, 0].view(len(SPECIAL), 3) * (ref['w'] + 1) / 2.0
    assert float(d[:, 0].abs().max()) == 0.0                       # ignored points
    assert float(d[4:, 1:].abs().max()) <= 1e-30                   # +-100: clamped value, no gradient
    assert abs(float(d[3, 2]) + 4.25e-06) < 1e-7                   # -40, y = 1: (p - y) / 1e-12 * p (1 - p)


# ------------------------------------------------------------------------------------------------ model level
@pytest.mark.parametrize('case', sorted(GT.CASES))
def test_forward_train_losses_match_reference_with_fused_losses(case, monkeypatch):
    monkeypatch.setattr(SoftGroup, 'use_fused_losses', True)
    model, batch, ref, seed = _train_case(case)
    model.train()
    torch.manual_seed(seed)
    loss, log_vars = model(batch, return_loss=True)
    print(case, {k: (round(log_vars[k], 6), round(ref[k], 6)) for k in ref})
    assert list(log_vars) == list(ref)
    for k, want in ref.items():
        got = log_vars[k]
        if k.startswith('num_'):
            assert got == want, (k, got, want)
        else:
            assert abs(got - want) <= LOSS_RTOL * max(abs(want), 1e-3), (k, got, want)
    assert abs(float(loss) - ref['loss']) <= LOSS_RTOL * abs(ref['loss'])


def test_forward_train_gradients_equal_with_switch_on_and_off(monkeypatch):
    """s3dis_fold5, same batch, weights and seed: the forward pass is the same in both runs, so every trainable
    tensor's gradient agrees within 1e-4 of its largest entry plus the 1e-5 floor of the largest entry overall"""
    model, batch, ref, seed = _train_case('s3dis_fold5')
    model.train()
    grads = {}
    for on in (False, True):
        monkeypatch.setattr(SoftGroup, 'use_fused_losses', on)
        model.zero_grad(set_to_none=True)
        torch.manual_seed(seed)
        loss, _ = model(batch, return_loss=True)
        loss.backward()
        grads[on] = {n: (None if p.grad is None else p.grad.detach().double().cpu())
                     for n, p in model.named_parameters() if p.requires_grad}
    assert grads[False] and set(grads[False]) == set(grads[True])
    floor = 1e-5 * max(float(g.abs().max()) for g in grads[False].values() if g is not None)
    worst = []
    for n, want in grads[False].items():
        got = grads[True][n]
        assert (got is None) == (want is None), n
        if want is None:
            continue
        scale = float(want.abs().max())
        err = float((got - want).abs().max())
        worst.append((err / max(scale, 1e-30), n))
        assert err <= 1e-4 * scale + floor, (n, err, scale, floor)
    print('worst relative differences', sorted(worst, reverse=True)[:3])


def test_bf16_autocast_step_with_fused_losses(monkeypatch):
    """one bf16-autocast step on the fused losses: finite, every term within 2 % (+ 5e-3) of the fp32 step from the
    same weights on the same proposals -- the bound of test_bf16_autocast_losses_explained[scannet_frozen]"""
    monkeypatch.setattr(SoftGroup, 'use_fused_losses', True)
    model, batch, ref, seed = _train_case('scannet_frozen')
    model.train()
    model.use_native_scan = False
    keep = {}
    orig = model.forward_grouping

    def record(*a, **k):
        keep['p'] = orig(*a, **k)
        return keep['p']

    model.forward_grouping = record
    torch.manual_seed(seed)
    _, fp32 = model(batch, return_loss=True)
    p32 = keep['p']
    model.forward_grouping = lambda *a, **k: p32
    torch.manual_seed(seed)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        loss, bf16 = model(batch, return_loss=True)
    loss.backward()
    print('fp32', fp32, '\nbf16', bf16)
    assert all(np.isfinite(v) for v in bf16.values())
    grads = [p.grad for p in model.parameters() if p.requires_grad and p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)
    for k, want in fp32.items():
        if k.startswith('num_'):
            assert bf16[k] == want
        else:
            assert abs(bf16[k] - want) <= 0.02 * abs(want) + 5e-3, (k, bf16[k], want)
