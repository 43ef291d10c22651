"""The inference U-Net executor (csrc/unet_exec.hip, sg_unet_forward) and the module path, EACH ON ITS OWN against
the float64 eval-mode reference of tests/unet_train_ref.py (EvalReference: gather tables from the CPU oracle, one
float64 matmul per kernel offset, BatchNorm on the running statistics) -- the inference-side counterpart of
tests/test_unet_train_ref_gpu.py.  test_unet_executor_*, test_plan_modes_gpu.py and test_conv_chain_gpu.py compare
the executor with the module path, chains on with chains off: both sides launch the same kernels, and a fault they
share cancels.  Here the other side is plain torch.

Nets (random running statistics and affine parameters):
  small3   [16, 32, 48] x 2 blocks, odd extents [45, 37, 29], batch 2: no chain, fragment-shaped gather (16, 48)
  input6   [32, 64, 96] behind a 6-channel input conv (padded to 16 channels), ~3 000 rows: chain below the input conv
  scannet7 32 .. 224 over 7 levels at ~6 000 rows: deep levels of 40 rows down to none (odd-extent drop), offset-split
           layers, the 96 / 160 / 224-channel row pitches
  one3     one level, 3 blocks: the stray BatchNorm + ReLU step
each in arithmetic 0 (fp32 MFMA) and 1 (split precision), the executor with conv chains on and off.  Arithmetic 2
is not compared at this level: activations that differ in the last fp32 bit round to different bf16 values, the
bar would be a guess; tests/test_conv_ref_gpu.py covers it layer by layer.

Bar: the project's rule for a forward tensor in the maximum norm, 1e-4 of the largest reference entry (group (a) of
test_unet_train_ref_gpu.py).  The same reference evaluated in float32 torch ops is measured alongside and printed.

Measured on an MI355X, max |got - ref| / max |ref|:

  net       arith  float32 torch  chains on  chains off  module path   rows per level
  small3        0       2.62e-07   1.49e-07    1.49e-07     3.45e-07   [4353, 1566, 416]
  small3        1       2.62e-07   2.36e-07    2.36e-07     3.45e-07   [4353, 1566, 416]
  input6        0       3.60e-07   1.47e-07    1.47e-07     2.61e-07   [2809, 796, 181]
  input6        1       3.60e-07   1.92e-07    1.92e-07     2.79e-07   [2809, 796, 181]
  scannet7      0       3.59e-07   2.04e-07    2.04e-07     3.59e-07   [5839, 2929, 799, 209, 36, 6, 0]
  scannet7      1       3.59e-07   1.83e-07    1.83e-07     3.33e-07   [5839, 2929, 799, 209, 36, 6, 0]
  one3          0       1.20e-07   9.18e-08    9.18e-08     9.18e-08   [1570]
  one3          1       1.20e-07   8.74e-08    8.74e-08     8.74e-08   [1570]
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_train_ref as R  # noqa: E402

import softgroup_amd.spconv.pytorch as spconv  # noqa: E402
from softgroup_amd.model.blocks import ResidualBlock, UBlock  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BAR = 1e-4

#        name       planes                      reps cin   points extent        batch
NETS = {
    'small3': ([16, 32, 48], 2, None, 6000, [45, 37, 29], 2),
    'input6': ([32, 64, 96], 2, 6, 4800, [41, 37, 25], 1),
    'scannet7': ([32 * i for i in range(1, 8)], 2, None, 7000, [97, 75, 45], 1),
    'one3': ([32], 3, None, 2500, [33, 29, 21], 1),
}


class Net(nn.Module):
    """input conv (optional), UBlock, output BatchNorm + ReLU: the module names of EvalReference's state dict"""

    def __init__(self, planes, cin, reps):
        super().__init__()
        norm_fn = functools.partial(nn.BatchNorm1d, eps=1e-4, momentum=0.1)
        self.input_conv = None
        if cin is not None:
            self.input_conv = spconv.SparseSequential(
                spconv.SubMConv3d(cin, planes[0], kernel_size=3, padding=1, bias=False, indice_key='subm1'))
        self.unet = UBlock(planes, norm_fn, reps, ResidualBlock, indice_key_id=1)
        self.output_layer = spconv.SparseSequential(norm_fn(planes[0]), nn.ReLU())


def _randomise_bn(mods):
    for m in mods:
        if isinstance(m, nn.BatchNorm1d):
            with torch.no_grad():
                m.running_mean.normal_(0, 0.3)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.normal_(1, 0.2)
                m.bias.normal_(0, 0.2)


@functools.lru_cache(maxsize=None)
def _setup(name):
    """the net, its input and the two evaluations of the reference (computed once per net, never changed)"""
    planes, reps, cin, points, extent, batch = NETS[name]
    torch.manual_seed(len(name) + points)
    net = Net(planes, cin, reps).eval()
    _randomise_bn(net.modules())
    idx = R.surface_voxels(np.random.default_rng(points), points, extent, batch)
    feats = torch.randn(len(idx), cin or planes[0])
    ref = R.EvalReference(net.state_dict(), idx, extent, batch)
    want = ref.forward(feats)
    want32 = ref.forward(feats, dtype=torch.float32)
    return net.to(DEV), idx, feats, ref.level_rows, want, want32


def _chain_launches():
    import ctypes as C
    from softgroup_amd import _lib as L
    a, b = C.c_int64(0), C.c_int64(0)
    L.check(L.lib().sg_spconv_chain_stats(C.byref(a), C.byref(b)), 'sg_spconv_chain_stats')
    return a.value


def _dist(got, want):
    return float((got.detach().cpu().double() - want).abs().max()) / float(want.abs().max())


@pytest.mark.parametrize('arith', [0, 1])
@pytest.mark.parametrize('name', list(NETS))
def test_executor_and_module_path_against_float64(name, arith):
    from softgroup_amd import _lib as L
    from softgroup_amd.spconv import unet_exec
    lib = L.lib()
    net, idx, feats, level_rows, want, want32 = _setup(name)
    planes, reps, cin, points, extent, batch = NETS[name]
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0.1 and float((want > 0).double().mean()) > 0.2
    if name == 'scannet7':
        assert len(level_rows) == 7 and 5000 <= level_rows[0] <= 7000 and level_rows[-1] == 0, level_rows
        assert any(1 <= r <= 40 for r in level_rows), level_rows
    if name == 'input6':
        assert 2500 <= level_rows[0] <= 3600, level_rows
    x = spconv.SparseConvTensor(feats.to(DEV), torch.from_numpy(idx).to(DEV), extent, batch)
    ex = unet_exec.UNetExecutor(net.unet, net.input_conv, net.output_layer)
    got = {}
    try:
        L.check(lib.sg_spconv_set_arithmetic(arith), 'sg_spconv_set_arithmetic')
        with torch.no_grad():
            assert ex.usable(x.features)
            for chain in (1, 0):
                L.check(lib.sg_spconv_set_chain(chain), 'sg_spconv_set_chain')
                before = _chain_launches()
                got[f'executor, chains {"on" if chain else "off"}'] = ex(x).clone()
                torch.cuda.synchronize()
                launched = _chain_launches() - before
                assert launched == 0 if not chain else launched >= 1 or name not in ('input6', 'scannet7'), (chain, launched)
            h = net.input_conv(x) if net.input_conv is not None else x
            got['module path'] = net.output_layer(net.unet(h)).features.clone()
        torch.cuda.synchronize()
    finally:
        lib.sg_spconv_set_chain(-1)
        lib.sg_spconv_set_arithmetic(-1)
    e32 = _dist(want32, want)
    dist = {k: _dist(v, want) for k, v in got.items()}
    print(f'{name:9s} arith {arith} rows {level_rows}: float32 torch {e32:.2e}  '
          + '  '.join(f'{k} {d:.2e}' for k, d in dist.items()))
    for k, v in got.items():
        assert v.shape == want.shape and torch.isfinite(v).all(), k
        assert dist[k] <= BAR, f'{name}, arithmetic {arith}, {k}: {dist[k]:.3e} of the largest reference entry'
