"""Fused loss block (softgroup_amd/ops/losses.py over csrc/losses.hip), the parts that need no GPU: the C ABI
carries the entries, the Python functions on CPU tensors equal torch's own losses (value and gradient) and the
reference's assignment loop (softgroup/model/softgroup.py:152-255), and bad arguments are refused by name."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from softgroup_amd import _lib, ops
from test_losses_cpu import _reference_labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ['sg_loss_reduce_workspace_bytes', 'sg_pointwise_loss_fwd', 'sg_pointwise_loss_bwd',
           'sg_assign_proposals_workspace_bytes', 'sg_assign_proposals', 'sg_proposal_loss_fwd',
           'sg_proposal_loss_bwd', 'sg_mask_loss_fwd', 'sg_mask_loss_bwd']


def test_entries_are_in_header_table_and_library():
    txt = open(os.path.join(ROOT, 'include', 'softgroup_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    declared = set(re.findall(r'\b(sg_[a-z0-9_]+)\s*\(', txt))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(raw, name), name
    assert set(_lib.SIGNATURES) == declared


def test_switch_is_off_by_default():
    from softgroup_amd.model import SoftGroup
    assert SoftGroup.use_fused_losses is (os.environ.get('SG_FUSED_LOSSES', '0') == '1')


@pytest.mark.parametrize('n,c', [(1000, 13), (257, 20), (5, 3), (64, 1)])
def test_point_wise_loss_cpu_equals_torch(n, c):
    torch.manual_seed(n + c)
    for weight in (None, torch.rand(c) + 0.1):
        s = torch.randn(n, c, requires_grad=True)
        o = torch.randn(n, 3, requires_grad=True)
        ol = torch.randn(n, 3)
        y = torch.randint(0, c, (n, ))
        y[::7] = -100
        y[1 % n] = 0
        inst = torch.randint(0, 5, (n, ))
        inst[::3] = -100
        inst[1 % n] = 2
        sem, off = ops.point_wise_loss(s, o, y, inst, ol, weight, -100)
        pos = inst != -100
        want_sem = F.cross_entropy(s, y, weight=weight, ignore_index=-100)
        want_off = F.l1_loss(o[pos], ol[pos], reduction='sum') / pos.sum()
        # float32 on both sides: a few ulp of the log-softmax and of the summation order
        assert abs(float(sem) - float(want_sem)) <= 1e-6 * max(abs(float(want_sem)), 1.0)
        assert abs(float(off) - float(want_off)) <= 1e-6 * max(abs(float(want_off)), 1.0)
        got = torch.autograd.grad(0.7 * sem + 1.3 * off, (s, o))
        want = torch.autograd.grad(0.7 * want_sem + 1.3 * want_off, (s, o))
        for a, b in zip(got, want):
            assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())
    # no instance point: 0, with a zero gradient (softgroup.py:164-165)
    _, off = ops.point_wise_loss(s, o, y, torch.full((n, ), -100), ol, None, -100)
    assert float(off) == 0.0 and float(torch.autograd.grad(off, o)[0].abs().max()) == 0.0


def test_assign_proposals_cpu_equals_the_reference_loop():
    g = torch.Generator().manual_seed(3)
    checked = 0
    for trial in range(100):
        n_prop = int(torch.randint(1, 14, (1, ), generator=g))
        n_gt = int(torch.randint(1, 10, (1, ), generator=g))
        ious = torch.rand(n_prop, n_gt, generator=g)
        ious[torch.rand(n_prop, n_gt, generator=g) < 0.35] = 0
        cls = torch.randint(0, 6, (n_gt, ), generator=g)
        cls[torch.rand(n_gt, generator=g) < 0.3] = -100
        if int((cls != -100).sum()) == 0:
            continue
        for mlq in (False, True):
            want = _reference_labels(ious, cls, 0.5, mlq, 0.1, 18)
            got = ops.assign_proposals(ious, cls, -100, 0.5, mlq, 0.1, 18)
            assert torch.equal(want, got), (trial, mlq)
            checked += 1
    assert checked > 100


def test_instance_losses_cpu_equal_torch():
    torch.manual_seed(5)
    P, G, K, M = 9, 5, 4, 200
    cls_scores = torch.randn(P, K + 1, dtype=torch.float64, requires_grad=True)
    iou_scores = torch.randn(P, K + 1, dtype=torch.float64, requires_grad=True)
    mask_scores = (3 * torch.randn(M, K + 1, dtype=torch.float64)).requires_grad_(True)
    labels = torch.randint(0, K + 1, (P, ))
    labels[0], labels[1] = K, 0
    bidx = torch.randint(0, P, (M, ), dtype=torch.int32)
    mask_label = torch.randint(-1, 2, (M, )).double()
    instance_cls = torch.tensor([1, -100, 0, 3, -100])
    ious = torch.rand(P, G, dtype=torch.float64)
    seen = {}

    def iou_on_pred(sig):
        seen['sig'] = sig
        return ious

    got = ops.instance_losses(cls_scores, mask_scores, iou_scores, labels, bidx, mask_label, instance_cls,
                              iou_on_pred, -100, K)
    assert list(got) == ['cls_loss', 'mask_loss', 'iou_score_loss', 'num_pos', 'num_neg']
    rows = torch.arange(M)
    sig = mask_scores.sigmoid()[rows, labels[bidx.long()]]
    assert torch.equal(seen['sig'], sig.detach()) and not seen['sig'].requires_grad
    w = (mask_label != -1).double()
    y = mask_label.clone()
    y[mask_label == -1] = 0.5
    want = dict(cls_loss=F.cross_entropy(cls_scores, labels),
                mask_loss=F.binary_cross_entropy(sig, y, weight=w, reduction='sum') / (w.sum() + 1))
    gt = ious[:, instance_cls != -100].max(1)[0]
    wi = (labels < K).double()
    want['iou_score_loss'] = (F.mse_loss(iou_scores[torch.arange(P), labels], gt, reduction='none') * wi).sum() / (wi.sum() + 1)
    for k, v in want.items():
        assert abs(float(got[k]) - float(v)) <= 1e-12 * max(abs(float(v)), 1.0), k
    assert float(got['num_pos']) == float((labels < K).sum()) and float(got['num_neg']) == float((labels >= K).sum())
    tensors = (cls_scores, mask_scores, iou_scores)
    a = torch.autograd.grad(got['cls_loss'] + 2 * got['mask_loss'] + 3 * got['iou_score_loss'], tensors)
    b = torch.autograd.grad(want['cls_loss'] + 2 * want['mask_loss'] + 3 * want['iou_score_loss'], tensors)
    for x, y_ in zip(a, b):
        assert float((x - y_).abs().max()) <= 1e-12


def test_bad_arguments_are_refused_by_name():
    lib = _lib.lib()
    one = ctypes.c_void_p(256)      # (never dereferenced: every call below fails its argument check first)
    calls = {
        'sg_pointwise_loss_fwd': [
            lambda: lib.sg_pointwise_loss_fwd(one, one, None, -100, one, one, one, -1, 13, one, one, 1 << 20, None),
            lambda: lib.sg_pointwise_loss_fwd(one, one, None, -100, one, one, one, 10, 0, one, one, 1 << 20, None),
            lambda: lib.sg_pointwise_loss_fwd(one, one, None, -100, one, one, one, 10, 65, one, one, 1 << 20, None),
            lambda: lib.sg_pointwise_loss_fwd(None, one, None, -100, one, one, one, 10, 13, one, one, 1 << 20, None),
            lambda: lib.sg_pointwise_loss_fwd(one, one, None, -100, one, one, one, 10, 13, one, one, 8, None)],
        'sg_pointwise_loss_bwd': [
            lambda: lib.sg_pointwise_loss_bwd(one, one, None, -100, one, one, one, -1, 13, one, one, one, one, one, None),
            lambda: lib.sg_pointwise_loss_bwd(one, one, None, -100, one, one, one, 10, 13, None, one, one, one, one, None),
            lambda: lib.sg_pointwise_loss_bwd(one, one, None, -100, one, one, one, 10, 100, one, one, one, one, one, None)],
        'sg_assign_proposals': [
            lambda: lib.sg_assign_proposals(one, one, -100, 0.5, 0, 0.0, 18, -1, 3, one, None, 0, None),
            lambda: lib.sg_assign_proposals(one, one, -100, 0.5, 0, 0.0, 18, 4, 0, one, None, 0, None),
            lambda: lib.sg_assign_proposals(None, one, -100, 0.5, 0, 0.0, 18, 4, 3, one, None, 0, None),
            lambda: lib.sg_assign_proposals(one, one, -100, 0.5, 1, 0.0, 18, 4, 3, one, None, 0, None)],
        'sg_proposal_loss_fwd': [
            lambda: lib.sg_proposal_loss_fwd(one, one, one, one, one, -100, 4, 3, 1, one, one, one, 1 << 20, None),
            lambda: lib.sg_proposal_loss_fwd(one, one, one, one, one, -100, 4, 3, 65, one, one, one, 1 << 20, None),
            lambda: lib.sg_proposal_loss_fwd(one, one, one, one, one, -100, -4, 3, 19, one, one, one, 1 << 20, None),
            lambda: lib.sg_proposal_loss_fwd(one, None, one, one, one, -100, 4, 3, 19, one, one, one, 1 << 20, None)],
        'sg_proposal_loss_bwd': [
            lambda: lib.sg_proposal_loss_bwd(one, one, one, one, one, one, one, 4, 1, one, one, None),
            lambda: lib.sg_proposal_loss_bwd(one, one, one, None, one, one, one, 4, 19, one, one, None)],
        'sg_mask_loss_fwd': [
            lambda: lib.sg_mask_loss_fwd(one, one, one, one, -1, 4, 19, one, one, one, 1 << 20, None),
            lambda: lib.sg_mask_loss_fwd(one, one, one, one, 10, 4, 70, one, one, one, 1 << 20, None),
            lambda: lib.sg_mask_loss_fwd(one, one, one, one, 10, 4, 19, None, one, one, 1 << 20, None)],
        'sg_mask_loss_bwd': [
            lambda: lib.sg_mask_loss_bwd(one, one, one, one, one, one, 10, 4, 1, one, None),
            lambda: lib.sg_mask_loss_bwd(one, one, one, one, one, one, 10, 4, 19, None, None)],
    }
    for name, bad in calls.items():
        for i, call in enumerate(bad):
            rc = call()
            assert rc < 0 and name.encode() in lib.sg_last_error(), (name, i, rc, lib.sg_last_error())
    assert lib.sg_loss_reduce_workspace_bytes() > 0
    assert lib.sg_assign_proposals_workspace_bytes(300) >= 2 * 300 * 4
