"""float64 reference of ONE layer of the inference convolution (csrc/spconv_conv.hip), exactly as the header
comment of that file states it:

    out[j, :] = post( residual[j, :] + sum_k in[nbr[j, k], :] . W[k] ),     post = relu(x * s + b) | id
    out_act   = relu(out * act_scale + act_shift)                            (optional second output)

Test helper.  Nothing here touches the HIP library: the layer is a gather and one matmul per kernel offset in
plain torch, on whatever device the operands live on (float64 on the device is still plain torch), and the
gather tables come from the CPU oracle -- ``oracle.subm_rulebook`` (K = 27), ``oracle.down_rulebook``'s child
table (K = 8, strided), the parity construction of ``unet_train_ref.Reference.__init__`` (K = 8, inverse) and
``arange`` (K = 1) -- never from the HIP rulebooks.

Besides the outputs ``layer`` returns what a rounding-error bound needs, per output element: ``s_out`` /
``s_act``, the sum of the absolute values of everything that is added up on the way to that output
(``S_abs = sum |in| . |W|`` carried through the epilogues: + |residual|, * |s| + |b|, * |act_scale| +
|act_shift|), and per row ``n``, the number of products of one of its elements (present taps x Cin).  With
unit roundoff u = 2^-24 any fp32 evaluation, in any summation order, stays within (n + ops) u S of the exact
value, where ``ops`` counts the epilogue's own roundings (``Layer.ops_out`` / ``ops_act``: one for the
residual add, two for each scale-and-shift).

For the training kernels (csrc/spconv_train.hip): ``round_bf16`` puts a float64 tensor on the bf16 grid with ONE
rounding (the kernel rounds an fp32 sum once; double -> float -> bf16 would round twice next to a midpoint),
``wgrad`` is the weight gradient dW[k] = X_k^T G and ``input_grad`` the scatter form of the layer's transpose,
each with its S_abs and its product counts.
"""
import os
import sys
from collections import namedtuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F64 = torch.float64
U32 = 2.0 ** -24            # unit roundoff of fp32

Layer = namedtuple('Layer', 'out out_act s_out s_act n ops_out ops_act')


# ---------------------------------------------------------------------------------------------------
# gather tables (CPU oracle)
# ---------------------------------------------------------------------------------------------------
def subm_table(idx, shape):
    """K = 27: [M, 27] input row per kernel offset, -1 = no neighbour"""
    import oracle
    return oracle.subm_rulebook(np.ascontiguousarray(idx, np.int32), [int(s) for s in shape])


def down_tables(idx, shape):
    """K = 8 pair of a level: (child [M_out, 8] of the strided conv, up [M, 8] of the inverse conv, M_out).
    up: fine row i takes offset k = parity of its coordinate from its parent (one tap, none for a row on a
    dropped odd last plane) -- the construction of unet_train_ref.Reference.__init__"""
    import oracle
    idx = np.ascontiguousarray(idx, np.int32)
    out_idx, in2out, child, _ = oracle.down_rulebook(idx, [int(s) for s in shape])
    k = (idx[:, 1] & 1) * 4 + (idx[:, 2] & 1) * 2 + (idx[:, 3] & 1)
    up = np.full((len(idx), 8), -1, np.int32)
    up[np.arange(len(idx)), k] = in2out
    return child, up, len(out_idx)


def identity_table(rows):
    """K = 1: the 1x1 shortcut conv"""
    return np.arange(rows, dtype=np.int32)[:, None]


# ---------------------------------------------------------------------------------------------------
# the layer
# ---------------------------------------------------------------------------------------------------
def _gathered_matmul(x, w, table):
    """sum_k x[table[:, k]] @ w[:, k].T with absent taps reading a zero row; x [N, Cin], w [Cout, K, Cin]"""
    n_in = x.shape[0]
    xp = torch.cat([x, x.new_zeros(1, x.shape[1])])                     # row n_in = absent neighbour
    out = x.new_zeros((table.shape[0], w.shape[0]))
    for k in range(table.shape[1]):
        rows = table[:, k]
        out += xp[torch.where(rows >= 0, rows, torch.full_like(rows, n_in))] @ w[:, k].t()
    return out


def layer(x, w, table, residual=None, post=None, act=None, dtype=F64, bounds=True):
    """x [N_in, Cin], w [Cout, K, Cin], table [M_out, K] (numpy or tensor, -1 = absent), residual [M_out, Cout],
    post = (scale, shift), act = (scale, shift); operands are converted to `dtype` as they are (round them
    beforehand for a reduced-precision arithmetic).  -> Layer; the bound quantities are float64 whatever
    `dtype` is (bounds=False: left out, s_out = s_act = None)."""
    dev = x.device
    table = torch.as_tensor(np.ascontiguousarray(table) if isinstance(table, np.ndarray) else table).to(dev).long()
    assert table.ndim == 2 and table.shape[1] == w.shape[1] and w.shape[2] == x.shape[1]
    assert int(table.max()) < x.shape[0] and int(table.min()) >= -1
    out = _gathered_matmul(x.to(dtype), w.to(dtype), table)
    s = _gathered_matmul(x.to(F64).abs(), w.to(F64).abs(), table) if bounds else None
    n = (table >= 0).sum(1) * x.shape[1]
    ops = 0
    if residual is not None:
        out = out + residual.to(dtype)
        s = s + residual.to(F64).abs() if bounds else None
        ops += 1
    if post is not None:
        out = torch.relu(out * post[0].to(dtype) + post[1].to(dtype))
        s = s * post[0].to(F64).abs() + post[1].to(F64).abs() if bounds else None
        ops += 2
    out_act = s_act = None
    if act is not None:
        out_act = torch.relu(out * act[0].to(dtype) + act[1].to(dtype))
        s_act = s * act[0].to(F64).abs() + act[1].to(F64).abs() if bounds else None
    return Layer(out, out_act, s, s_act, n, ops, ops + 2)


def dense_loop(x, w, table):
    """the same sum written as the three-line loop it is (numpy float64; small inputs only)"""
    out = np.zeros((table.shape[0], w.shape[0]))
    for j in range(table.shape[0]):
        for k in range(table.shape[1]):
            if table[j, k] >= 0:
                out[j] += w[:, k, :].astype(np.float64) @ x[table[j, k]].astype(np.float64)
    return out


# ---------------------------------------------------------------------------------------------------
# the training side: bf16 grid, weight gradient, input gradient
# ---------------------------------------------------------------------------------------------------
BF16_MAX = (2.0 - 2.0 ** -7) * 2.0 ** 127


def round_bf16(x):
    """float64 -> nearest bf16 value (ties to even), as float64, rounded ONCE and in float64: x = m 2^e with
    0.5 <= |m| < 1 (frexp), the 8 significant bits of bf16 are round(m 2^8), scaled back by ldexp.  Below the
    smallest normal (2^-126) the grid has the fixed spacing 2^-133; above the largest finite value the result
    is +-inf, as in the float32 -> bf16 conversion; inf and NaN pass through."""
    x = x.to(F64)
    m, e = torch.frexp(x)
    e = e.long().clamp(-200, 200)                     # (beyond: 0 or inf either way; keeps 2^k a normal double)
    lift = (-125 - e).clamp(min=0)                    # subnormal range: fewer than 8 bits are left
    q = torch.round(_ldexp(torch.where(x.abs() < 2.0 ** -150, torch.zeros_like(x), m), 8 - lift))
    r = torch.copysign(_ldexp(q, e + lift - 8), x)    # (a zero keeps the sign of x)
    r = torch.where(r.abs() > BF16_MAX, torch.copysign(torch.full_like(r, float('inf')), x), r)
    return torch.where(torch.isfinite(x), r, x)


def _ldexp(v, k):
    """v 2^k, exact: 2^k is put together from its bits (torch.ldexp multiplies by pow(2, k), which a device's
    pow need not return exactly)"""
    return v * ((k + 1023) << 52).view(F64)


def _table(table, dev):
    return torch.as_tensor(np.ascontiguousarray(table) if isinstance(table, np.ndarray) else table).to(dev).long()


def wgrad(x, g, table):
    """dW[k] = X_k^T G over the existing (row, offset) pairs: x [N_in, Cin], g [M_out, Cout], table [M_out, K]
    -> (dW [K, Cin, Cout] float64, S_abs [K, Cin, Cout] = |X_k|^T |G|, n [K] = pairs of offset k)"""
    table = _table(table, x.device)
    assert table.ndim == 2 and table.shape[0] == g.shape[0] and int(table.max()) < x.shape[0]
    x, g = x.to(F64), g.to(F64)
    K = table.shape[1]
    dw = x.new_zeros((K, x.shape[1], g.shape[1]))
    s = torch.zeros_like(dw)
    n = torch.zeros(K, dtype=torch.long, device=x.device)
    for k in range(K):
        j = torch.nonzero(table[:, k] >= 0)[:, 0]
        xk, gk = x[table[j, k]], g[j]
        dw[k] = xk.t() @ gk
        s[k] = xk.abs().t() @ gk.abs()
        n[k] = j.numel()
    return dw, s, n


def input_grad(g, w, table, n_in):
    """the layer's transpose as a scatter: dX[table[j, k]] += g[j] @ w[:, k, :]; g [M_out, Cout], w [Cout, K, Cin]
    -> (dX [n_in, Cin] float64, S_abs [n_in, Cin], n [n_in] = products of one element of that row: pairs x Cout)"""
    table = _table(table, g.device)
    assert table.ndim == 2 and table.shape[0] == g.shape[0] and table.shape[1] == w.shape[1] and w.shape[0] == g.shape[1]
    g, w = g.to(F64), w.to(F64)
    dx = g.new_zeros((n_in, w.shape[2]))
    s = torch.zeros_like(dx)
    n = torch.zeros(n_in, dtype=torch.long, device=g.device)
    for k in range(table.shape[1]):
        j = torch.nonzero(table[:, k] >= 0)[:, 0]
        dst = table[j, k]
        dx.index_add_(0, dst, g[j] @ w[:, k, :])
        s.index_add_(0, dst, g[j].abs() @ w[:, k, :].abs())
        n.index_add_(0, dst, torch.full_like(dst, w.shape[0]))
    return dx, s, n


def wgrad_loop(x, g, table):
    """wgrad as the plain triple loop (numpy float64; small inputs only)"""
    dw = np.zeros((table.shape[1], x.shape[1], g.shape[1]))
    for j in range(table.shape[0]):
        for k in range(table.shape[1]):
            if table[j, k] >= 0:
                dw[k] += np.outer(x[table[j, k]].astype(np.float64), g[j].astype(np.float64))
    return dw


def input_grad_loop(g, w, table, n_in):
    """input_grad as the plain triple loop (numpy float64; small inputs only)"""
    dx = np.zeros((n_in, w.shape[2]))
    for j in range(table.shape[0]):
        for k in range(table.shape[1]):
            if table[j, k] >= 0:
                dx[table[j, k]] += g[j].astype(np.float64) @ w[:, k, :].astype(np.float64)
    return dx
