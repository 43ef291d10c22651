"""Pins the float64 reference of the training U-Net (tests/unet_train_ref.py) itself, on the CPU: on
small grids it must equal the same network built from dense ``F.conv3d`` / ``F.conv_transpose3d`` with
active-site masks and ``nn.BatchNorm1d`` in float64 (the construction
tests/test_train_gpu.py::test_conv_gradients_match_dense_autograd uses) -- output, running statistics
and every gradient to 1e-10 relative.  The dense side finds its active sites by max-pooling the
occupancy mask: it shares neither the oracle's rulebooks nor the reference's gather loop.  Also here:
the ambiguity probe (counts, slack) on a constructed input, and the recount of the ambiguous units of
the committed GPU cases of group (a) (tests/test_unet_train_ref_gpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_train_ref as R  # noqa: E402
import test_unet_train_ref_gpu as T  # noqa: E402

F64 = torch.float64


def _dense_step(sd, idx, shape, batch, feats, g_out, eps=1e-4, momentum=0.1):
    """-> out, g_in, grads, buffers of the dense float64 network"""
    p = {k: v.to(F64).clone().requires_grad_(True) for k, v in sd.items()
         if v.is_floating_point() and 'running_' not in k}
    bns = {}

    def bn_relu(x, name):
        m = nn.BatchNorm1d(x.shape[1], eps=eps, momentum=momentum).double().train()
        del m._parameters['weight'], m._parameters['bias']      # the leaf tensors themselves, not copies
        m.weight, m.bias = p[name + '.weight'], p[name + '.bias']
        with torch.no_grad():
            m.running_mean.copy_(sd[name + '.running_mean'])
            m.running_var.copy_(sd[name + '.running_var'])
            m.num_batches_tracked.copy_(sd[name + '.num_batches_tracked'])
        bns[name] = m
        return F.relu(m(x))

    def to_dense(x, li, shp):
        d = x.new_zeros((batch, *shp, x.shape[1]))
        return d.index_put((li[:, 0], li[:, 1], li[:, 2], li[:, 3]), x).permute(0, 4, 1, 2, 3)

    def rows_of(d, li):
        return d[li[:, 0], :, li[:, 1], li[:, 2], li[:, 3]]

    def subm(x, name, li, shp):
        w = p[name + '.weight'].permute(0, 4, 1, 2, 3)
        return rows_of(F.conv3d(to_dense(x, li, shp), w, padding=1), li)

    def block(x, name, li, shp):
        cb = name + '.conv_branch.'
        h = subm(bn_relu(x, cb + '0'), cb + '2', li, shp)
        h = subm(bn_relu(h, cb + '3'), cb + '5', li, shp)
        ib = name + '.i_branch.0.weight'
        if ib in p:
            x = rows_of(F.conv3d(to_dense(x, li, shp), p[ib].permute(0, 4, 1, 2, 3)), li)
        return h + x

    def blocks(x, name, li, shp):
        i = 0
        while f'{name}.block{i}.conv_branch.0.weight' in p:
            x = block(x, f'{name}.block{i}', li, shp)
            i += 1
        return x

    def level(x, name, li, shp):
        x = blocks(x, name + 'blocks', li, shp)
        if name + 'conv.2.weight' not in p:
            return x
        occ = torch.zeros((batch, 1, *shp), dtype=F64)
        occ[li[:, 0], 0, li[:, 1], li[:, 2], li[:, 3]] = 1
        occ2 = F.max_pool3d(occ, 2, 2)                            # floor: an odd extent drops its last plane
        lo = torch.nonzero(occ2[:, 0] > 0)
        shp2 = [s // 2 for s in shp]
        d = F.conv3d(to_dense(bn_relu(x, name + 'conv.0'), li, shp), p[name + 'conv.2.weight'].permute(0, 4, 1, 2, 3),
                     stride=2)
        d = level(rows_of(d, lo), name + 'u.', lo, shp2)
        u = F.conv_transpose3d(to_dense(bn_relu(d, name + 'deconv.0'), lo, shp2),
                               p[name + 'deconv.2.weight'].permute(4, 0, 1, 2, 3), stride=2)
        u = F.pad(u, (0, shp[2] - u.shape[4], 0, shp[1] - u.shape[3], 0, shp[0] - u.shape[2]))
        return blocks(torch.cat([x, rows_of(u, li)], 1), name + 'blocks_tail', li, shp)

    li = torch.from_numpy(idx.astype(np.int64))
    x0 = feats.to(F64).clone().requires_grad_(True)
    x = x0
    if 'input_conv.0.weight' in p:
        x = subm(x, 'input_conv.0', li, list(shape))
    out = bn_relu(level(x, 'unet.', li, list(shape)), 'output_layer.0')
    out.backward(g_out.to(F64))
    buffers = {}
    for name, m in bns.items():
        buffers[name + '.running_mean'] = m.running_mean
        buffers[name + '.running_var'] = m.running_var
        buffers[name + '.num_batches_tracked'] = m.num_batches_tracked
    return out.detach(), x0.grad, {k: t.grad for k, t in p.items()}, buffers


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


DENSE_CASES = [
    # planes, cin, reps, extent, batch, occupancy
    ([8, 12], None, 1, [9, 7, 8], 2, 0.3),           # odd extents: the strided level drops the last planes
    ([8, 16, 12], 6, 2, [8, 8, 12], 1, 0.25),
    ([12], None, 3, [5, 6, 4], 3, 0.4),
    ([4, 8], None, 1, [6, 6, 6], 1, 0.2),
]


@pytest.mark.parametrize('planes,cin,reps,extent,batch,occ', DENSE_CASES, ids=[str(c[0]) for c in DENSE_CASES])
@pytest.mark.parametrize('checkpoint_rows', [50000, 0], ids=['plain', 'checkpointed'])
def test_reference_equals_dense_float64_network(planes, cin, reps, extent, batch, occ, checkpoint_rows):
    rng = np.random.default_rng(sum(planes) + reps)
    idx = np.argwhere(rng.random((batch, *extent)) < occ).astype(np.int32)
    idx = idx[rng.permutation(len(idx))]
    M = len(idx)
    torch.manual_seed(7)
    net = T.Net(planes, cin, reps).train()
    T.randomise(net, 11)
    sd = net.state_dict()
    feats = torch.randn(M, cin if cin is not None else planes[0], dtype=F64)
    g_out = torch.randn(M, planes[0], dtype=F64)
    ref = R.reference_step(sd, idx, extent, batch, feats, g_out, checkpoint_rows=checkpoint_rows)
    out, g_in, grads, buffers = _dense_step(sd, idx, extent, batch, feats, g_out)
    assert len(ref.level_rows) == len(planes) and ref.level_rows[-1] >= 2
    assert _rel(ref.out, out) <= 1e-10
    assert _rel(ref.g_in, g_in) <= 1e-10
    assert set(ref.grads) == set(grads) == {k for k, _ in net.named_parameters()}
    for k in grads:
        assert _rel(ref.grads[k], grads[k]) <= 1e-10, k
    assert set(ref.buffers) == set(buffers) == {k for k, _ in net.named_buffers()}
    for k in buffers:
        if k.endswith('num_batches_tracked'):
            assert int(ref.buffers[k]) == int(buffers[k]) == 1
        else:
            assert _rel(ref.buffers[k], buffers[k]) <= 1e-10, k


def test_frozen_tensors_get_no_gradient_and_leave_the_others_unchanged():
    rng = np.random.default_rng(3)
    extent, batch = [8, 8, 8], 2
    idx = np.argwhere(rng.random((batch, *extent)) < 0.3).astype(np.int32)
    torch.manual_seed(1)
    net = T.Net([8, 12], None, 1).train()
    T.randomise(net, 2)
    sd = net.state_dict()
    feats, g_out = torch.randn(len(idx), 8, dtype=F64), torch.randn(len(idx), 8, dtype=F64)
    full = R.reference_step(sd, idx, extent, batch, feats, g_out)
    frozen = [k for i, (k, _) in enumerate(net.named_parameters()) if i % 3 == 0]
    part = R.reference_step(sd, idx, extent, batch, feats, g_out, input_grad=False, frozen=frozen)
    assert part.g_in is None and set(part.grads) == set(full.grads) - set(frozen)
    for k in part.grads:
        assert torch.equal(part.grads[k], full.grads[k]), k


def test_probe_counts_ambiguous_units_and_measures_their_slack():
    """a one-level net whose LAST ReLU gets one pre-activation moved onto zero by hand: the probe must
    count exactly that unit, and the slack of the output BatchNorm's bias gradient must be that unit's
    upstream gradient"""
    rng = np.random.default_rng(9)
    extent, batch = [6, 6, 6], 1
    idx = np.argwhere(rng.random((batch, *extent)) < 0.4).astype(np.int32)
    torch.manual_seed(5)
    net = T.Net([8], None, 1).train()
    T.randomise(net, 6)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    feats, g_out = torch.randn(len(idx), 8, dtype=F64), torch.randn(len(idx), 8, dtype=F64)
    clean = R.reference_step(sd, idx, extent, batch, feats, g_out)
    assert clean.ambiguous == 0 and all(s == 0.0 for s in clean.slack.values())
    assert len(clean.relus) == 3 and clean.min_ratio() > R.GRAD_MARGIN
    # pre-activation (row 4, channel 2) of the last ReLU = weight * xhat + bias: choose the bias that zeroes it
    pre = {}
    R.reference_step(sd, idx, extent, batch, feats, g_out, keep_pre=pre)
    sd['output_layer.0.bias'] = sd['output_layer.0.bias'].to(F64)
    sd['output_layer.0.bias'][2] -= pre['output_layer.0'][4, 2]
    hit = R.reference_step(sd, idx, extent, batch, feats, g_out)
    assert hit.ambiguous == 1 and hit.relus['output_layer.0']['ambiguous'] == 1
    assert hit.relus['output_layer.0']['min_ratio'] < R.GRAD_MARGIN
    assert abs(hit.slack['output_layer.0.bias'] - abs(float(g_out[4, 2]))) <= 1e-12
    assert hit.slack['input'] > 0


def test_counter_block_boundary_is_derived_from_the_kernel_source():
    """the depth cases of the GPU test sit at the boundary computed from csrc/unet_train.hip's constants"""
    c = T.kernel_constants()
    assert c['kStatCounters'] == 1 + c['kStatBlocksMax'] // c['kStatGroup']
    fit = c['kCounters'] // c['kStatCounters']
    assert T.column_sums_calls(7, T.DEPTH_FIRST_PAST - 1) <= fit < T.column_sums_calls(7, T.DEPTH_FIRST_PAST)
    assert T.column_sums_calls(7, 2 * T.DEPTH_FIRST_PAST) > 2 * fit
    assert T.column_sums_calls(2, T.DEPTH_TWO_LEVEL_REPS - 1) <= fit < T.column_sums_calls(2, T.DEPTH_TWO_LEVEL_REPS)
    for name, c_, nb, rows in T.SHAPE_ROWS:
        assert T.stat_blocks(rows, c_) == nb, name
        assert T.stat_blocks(rows, c_, c['kStatBlocksMax']) == min(nb, c['kStatBlocksMax']), name
        case = {k['name']: k for k in T.SHAPE_CASES}[name]
        assert case['n'] == rows == case['level_rows'][0] and case['planes'] == [32, 64], name
        lanes = 256 // (c_ // 4)
        assert rows % (lanes * 4) != 0, name
    assert {32, 64} == {c_ for _, c_, _, _ in T.SHAPE_ROWS}
    assert sorted({nb for _, _, nb, _ in T.SHAPE_ROWS}) == [15, 16, 17, 511, 512, 514]
    big = T.SHAPE_CASES[-1]
    assert big['level_rows'][0] >= 300000 and len(big['planes']) == 2


@pytest.mark.parametrize('case', T.FLIP_FREE_CASES, ids=[c['name'] for c in T.FLIP_FREE_CASES])
def test_committed_flip_free_cases_have_no_ambiguous_unit(case):
    """the seeds of group (a) were searched with `python tests/unet_train_ref.py search a`; this recounts"""
    net, idx, feats, g_out = T.build_case(case)
    ref = R.reference_step(net.state_dict(), idx, case['extent'], case['batch'], feats, g_out,
                           **T.run_kwargs(case, net))
    assert ref.ambiguous == 0 and all(s == 0.0 for s in ref.slack.values())
    assert ref.level_rows == case['level_rows'], ref.level_rows
