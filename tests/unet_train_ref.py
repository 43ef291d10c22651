"""float64 reference of one training step of the sparse U-Net that tests/test_unet_train_gpu.py builds
(``Net``: optional input SubM conv, ``UBlock`` of ``ResidualBlock``s, output BatchNorm + ReLU) -- the
independent yardstick of the native training executor (csrc/unet_train.hip).  Test helper, CPU only.

Nothing here touches the HIP library: the gather tables come from the CPU oracle
(``oracle.subm_rulebook`` / ``oracle.down_rulebook``), a convolution is a gather and one float64
matmul per kernel offset, BatchNorm is written out (batch mean, biased variance, eps, affine; running
statistics with the unbiased variance and the momentum, as torch.nn.functional.batch_norm defines
them), gradients come from torch autograd.

ReLU ambiguity (the rule of tests/golden/make_ref_train.py): a pre-activation within ``GRAD_MARGIN`` of
the tensor's rms may take the other branch in an fp32 implementation.  Every ReLU records its smallest
|pre-activation| / rms and how many units lie below the margin; the backward runs a second time with
exactly those units inverted, and ``slack`` of a gradient tensor is how far it moved.  All of it is a
property of the reference alone.

    python tests/unet_train_ref.py            # recount the ambiguous units of every committed GPU case
    python tests/unet_train_ref.py search a   # look for flip-free seeds of group a / b / c
"""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch
from torch.utils.checkpoint import checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GRAD_MARGIN = 5e-6          # tests/golden/make_ref_train.py: GRAD_MARGIN, of the pre-activation's rms
F64 = torch.float64


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
def surface_voxels(rng, n, extent, batch):
    """~n points on a wavy sheet (the generator of tests/test_unet_train_gpu.py), unique voxels,
    -> int32 [M, 4] (batch, x, y, z), batch-sorted"""
    pts = rng.random((n, 3)) * extent
    pts[:, 2] = (np.sin(pts[:, 0] * 0.3) + np.cos(pts[:, 1] * 0.2)) * 3 + extent[2] / 2 + rng.normal(0, 0.6, n)
    v = np.clip(np.floor(pts), 0, np.array(extent) - 1).astype(np.int64)
    b = np.sort(rng.integers(0, batch, n))
    key = ((b * extent[0] + v[:, 0]) * extent[1] + v[:, 1]) * extent[2] + v[:, 2]
    _, first = np.unique(key, return_index=True)
    first = np.sort(first)
    return np.concatenate([b[first, None], v[first]], 1).astype(np.int32)


def exact_voxels(rng, rows, extent, batch):
    """exactly `rows` distinct voxels drawn uniformly from the grid, in random row order"""
    cells = batch * extent[0] * extent[1] * extent[2]
    assert rows <= cells
    key = rng.choice(cells, rows, replace=False)
    z = key % extent[2]
    y = key // extent[2] % extent[1]
    x = key // (extent[2] * extent[1]) % extent[0]
    b = key // (extent[2] * extent[1] * extent[0])
    return np.stack([b, x, y, z], 1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------
# ReLU with the ambiguity probe
# ---------------------------------------------------------------------------------------------------
class Probe:
    """shared by the ReLUs of one reference run"""

    def __init__(self, margin):
        self.margin, self.flip = margin, False
        self.relus = OrderedDict()          # name -> dict(units, ambiguous, min_ratio)


class _ProbeReLUFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, probe, name):
        ctx.save_for_backward(x)
        ctx.probe = probe
        rms = float(x.detach().pow(2).mean().sqrt())
        close = x.detach().abs() < probe.margin * max(rms, 1e-300)
        ctx.close = close if bool(close.any()) else None
        probe.relus[name] = dict(units=x.numel(), ambiguous=int(close.sum()),
                                 min_ratio=float(x.detach().abs().min()) / max(rms, 1e-300))
        return x.clamp(min=0)

    @staticmethod
    def backward(ctx, g):
        (x, ) = ctx.saved_tensors
        mask = x > 0
        if ctx.probe.flip and ctx.close is not None:
            mask = mask ^ ctx.close
        return g * mask.to(g.dtype), None, None


# ---------------------------------------------------------------------------------------------------
# the network
# ---------------------------------------------------------------------------------------------------
def _pairs(table):
    """gather table [rows_out, K] (-1: no neighbour) -> per offset k the (output rows, input rows)"""
    out = []
    for k in range(table.shape[1]):
        o = np.nonzero(table[:, k] >= 0)[0]
        if len(o):
            out.append((k, torch.from_numpy(o), torch.from_numpy(table[o, k].astype(np.int64))))
    return out


def _gather_conv(x, w, pairs, rows_out):
    """out[j] = sum_k W[:, k, :] . x[table[j, k]];  w: [Cout, K, Cin]"""
    out = x.new_zeros((rows_out, w.shape[0]))
    for k, o, i in pairs:
        out = out.index_add(0, o, x.index_select(0, i) @ w[:, k, :].t())
    return out


class Reference:
    """one forward + backward of ``Net`` in float64.  Attributes after ``run``:
    out, g_in (None without input gradient), grads (name -> tensor, frozen ones absent), buffers
    (running statistics and num_batches_tracked after the step), slack (name -> max |change| under the
    inverted ambiguous units; 'input' for the input gradient), relus, ambiguous, level_rows"""

    def __init__(self, state_dict, indices, spatial_shape, batch_size, eps=1e-4, momentum=0.1,
                 margin=GRAD_MARGIN, checkpoint_rows=50000, keep_pre=None):
        import oracle
        self.sd = {k: v.detach().cpu() for k, v in state_dict.items()}
        self.eps, self.momentum = eps, momentum
        self.probe = Probe(margin)
        self.checkpoint_rows = checkpoint_rows
        self.keep_pre = keep_pre            # dict: receives every ReLU's pre-activation
        idx = np.ascontiguousarray(np.asarray(indices, np.int32))
        assert idx.ndim == 2 and idx.shape[1] == 4 and 0 <= idx[:, 0].min() and idx[:, 0].max() < batch_size
        n_levels = 1
        while 'unet.' + 'u.' * (n_levels - 1) + 'conv.2.weight' in self.sd:
            n_levels += 1
        self.levels = []
        shape = [int(s) for s in spatial_shape]
        for l in range(n_levels):
            lv = dict(rows=len(idx), subm=_pairs(oracle.subm_rulebook(idx, shape)))
            if l + 1 < n_levels:
                out_idx, in2out, child, out_shape = oracle.down_rulebook(idx, shape)
                lv['down'] = _pairs(child)
                # inverse conv: fine row i takes offset k = parity of its coordinate from its parent
                k = (idx[:, 1] & 1) * 4 + (idx[:, 2] & 1) * 2 + (idx[:, 3] & 1)
                up = np.full((len(idx), 8), -1, np.int32)
                up[np.arange(len(idx)), k] = in2out
                lv['up'] = _pairs(up)
                idx, shape = np.ascontiguousarray(out_idx), out_shape
            self.levels.append(lv)
        self.level_rows = [lv['rows'] for lv in self.levels]

    # ---- layers
    def _conv(self, x, name, pairs, rows_out):
        w = self.p[name + '.weight']
        w = w.reshape(w.shape[0], -1, w.shape[-1])
        if max(rows_out, x.shape[0]) >= self.checkpoint_rows:      # (27 gathered copies per layer otherwise)
            return checkpoint(_gather_conv, x, w, pairs, rows_out, use_reentrant=False)
        return _gather_conv(x, w, pairs, rows_out)

    def _bn_relu(self, x, name):
        n = x.shape[0]
        mean = x.mean(0)
        var = (x - mean).pow(2).mean(0)                         # biased
        y = (x - mean) / torch.sqrt(var + self.eps) * self.p[name + '.weight'] + self.p[name + '.bias']
        m = self.momentum
        with torch.no_grad():
            self.buffers[name + '.running_mean'] = (1 - m) * self.sd[name + '.running_mean'].to(F64) + m * mean
            self.buffers[name + '.running_var'] = ((1 - m) * self.sd[name + '.running_var'].to(F64)
                                                   + m * var * (n / (n - 1.0)))
            self.buffers[name + '.num_batches_tracked'] = self.sd[name + '.num_batches_tracked'] + 1
        if self.keep_pre is not None:
            self.keep_pre[name] = y.detach().clone()
        return _ProbeReLUFn.apply(y, self.probe, name)

    def _block(self, x, name, lv):
        cb = name + '.conv_branch.'
        h = self._conv(self._bn_relu(x, cb + '0'), cb + '2', lv['subm'], lv['rows'])
        h = self._conv(self._bn_relu(h, cb + '3'), cb + '5', lv['subm'], lv['rows'])
        ib = name + '.i_branch.0.weight'
        if ib in self.p:
            w = self.p[ib]
            x = x @ w.reshape(w.shape[0], w.shape[-1]).t()
        return h + x

    def _blocks(self, x, name, lv):
        i = 0
        while f'{name}.block{i}.conv_branch.0.weight' in self.p:
            x = self._block(x, f'{name}.block{i}', lv)
            i += 1
        assert i >= 1
        return x

    def _level(self, x, l, name):
        lv = self.levels[l]
        x = self._blocks(x, name + 'blocks', lv)
        if l + 1 == len(self.levels):
            return x
        nxt = self.levels[l + 1]
        d = self._conv(self._bn_relu(x, name + 'conv.0'), name + 'conv.2', lv['down'], nxt['rows'])
        d = self._level(d, l + 1, name + 'u.')
        u = self._conv(self._bn_relu(d, name + 'deconv.0'), name + 'deconv.2', lv['up'], lv['rows'])
        return self._blocks(torch.cat([x, u], 1), name + 'blocks_tail', lv)

    # ---- the step
    def run(self, feats, g_out, input_grad=True, frozen=()):
        frozen = set(frozen)
        self.p, self.buffers = {}, {}
        for k, v in self.sd.items():
            if v.is_floating_point() and 'running_' not in k:
                self.p[k] = v.to(F64).clone().requires_grad_(k not in frozen)
        assert frozen <= set(self.p), frozen - set(self.p)
        x0 = feats.detach().cpu().to(F64).clone().requires_grad_(input_grad)
        g = g_out.detach().cpu().to(F64)
        x = x0
        if 'input_conv.0.weight' in self.p:
            x = self._conv(x, 'input_conv.0', self.levels[0]['subm'], self.levels[0]['rows'])
        out = self._bn_relu(self._level(x, 0, 'unet.'), 'output_layer.0')
        wanted = [('input', x0)] * input_grad + [(k, t) for k, t in self.p.items() if t.requires_grad]
        res = []
        for flip in (False, True):
            self.probe.flip = flip
            res.append(torch.autograd.grad(out, [t for _, t in wanted], g, retain_graph=not flip, allow_unused=True))
        self.probe.flip = False
        self.out = out.detach()
        self.relus = self.probe.relus
        self.ambiguous = sum(r['ambiguous'] for r in self.relus.values())
        self.grads, self.slack = {}, {}
        for (k, t), a, b in zip(wanted, *res):
            a = torch.zeros_like(t) if a is None else a
            b = torch.zeros_like(t) if b is None else b
            self.grads[k] = a
            self.slack[k] = float((a - b).abs().max()) if a.numel() else 0.0
        self.g_in = self.grads.pop('input', None)
        return self

    def min_ratio(self):
        return min(r['min_ratio'] for r in self.relus.values())


class EvalReference(Reference):
    """the eval-mode forward of the same net (the inference executor's yardstick, tests/test_unet_exec_ref_gpu.py):
    same tables, same layers and level walk; BatchNorm uses the running statistics with eps, the ReLU is plain (the
    forward is continuous in its inputs: no ambiguity probe) and there is no backward.  ``forward`` evaluates in
    `dtype` -- float64 is the reference, float32 the same plain torch ops at the precision of the kernels."""

    def _bn_relu(self, x, name):
        y = ((x - self.stats[name + '.running_mean']) / torch.sqrt(self.stats[name + '.running_var'] + self.eps)
             * self.p[name + '.weight'] + self.p[name + '.bias'])
        return y.clamp(min=0)

    def forward(self, feats, dtype=F64):
        self.p = {k: v.to(dtype) for k, v in self.sd.items() if v.is_floating_point() and 'running_' not in k}
        self.stats = {k: v.to(dtype) for k, v in self.sd.items() if 'running_' in k}
        with torch.no_grad():
            x = feats.detach().cpu().to(dtype)
            if 'input_conv.0.weight' in self.p:
                x = self._conv(x, 'input_conv.0', self.levels[0]['subm'], self.levels[0]['rows'])
            return self._bn_relu(self._level(x, 0, 'unet.'), 'output_layer.0')


def reference_step(state_dict, indices, spatial_shape, batch_size, feats, g_out, **kw):
    run_kw = {k: kw.pop(k) for k in ('input_grad', 'frozen') if k in kw}
    return Reference(state_dict, indices, spatial_shape, batch_size, **kw).run(feats, g_out, **run_kw)


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_unet_train_ref_gpu as T
    T.main(sys.argv[1:])
