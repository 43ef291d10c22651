"""Every launch form of the inference convolution (csrc/spconv_conv.hip), one layer at a time through
sg_spconv_gather_conv_f32, against the float64 reference of tests/conv_ref.py on gather tables from the CPU oracle.

The other tests of this kernel compare one kernel path with another (two arithmetics, two combine forms, chain
on / off, executor / module path): a fault both sides share cancels there.  Here nothing on the reference side
comes from the library, and every case first ASKS the library which form it is about to run
(sg_spconv_conv_launch_info, the launch path's own decision) and asserts that this is the form the case is named
for -- which form a shape reaches depends on CU count x occupancy, read at run time, so a retuned threshold or a
register change would otherwise move cases onto other kernels without anybody noticing.

Sizes: for each form the smallest number of output rows that selects it on this device (scan + bisection of the
query over M_out, then nudged until M_out % 32 is neither 0 nor 31), at most MAX_ROWS; voxels from
unet_train_ref.exact_voxels so the row count is exact.  If the named shape does not reach its form below the cap,
the other (K, Cin, Cout) of the channel lists of tests/golden/ref_configs.json are tried; if none does, the test
FAILS and names the form.  tests/test_conv_ref.py keeps CASES complete against the variant table in the source.

Tolerance, per output element and per output row, both against the float64 reference:
  * ceiling, any summation order:  |got - ref| <= (n + 8 + ops) 2^-24 S_abs.  n = products of the element, 8 covers
    the split's per-product error (O(2^-24 |ab|), `split3`), ops the roundings of the epilogue (conv_ref.layer),
    S_abs the sum of absolute values carried through the epilogue.  Arithmetic 2: the reference runs on operands
    rounded to bf16 (.bfloat16().double()); the products are then exact in fp32 and the same bound holds.
  * working bar: row error / the row's largest |ref| <= max(1e-5, 4 e32), e32 the same quantity of a plain float32
    torch evaluation of the same reference, measured per case (1e-5: the bar of
    test_split_precision_products_equal_fp32_mfma; 4: another summation order at the same precision).
Inputs: per-row magnitudes over 1e-3 .. 1e3.  Outputs are NaN-filled with poisoned spare rows behind them.

Measured on an MI355X (256 CUs), row error / row max, `plain` = no epilogue, `epi` = residual + post + act (the
larger of out and out_act); printed by every case:

  case                      K Cin->Cout  rows  form reported by the query                   plain   e32       epi     e32
  v0_2x2_lines_a1          27  64->64   49121  split 2x2 lines                              1.2e-06 8.2e-07   1.2e-06 7.8e-07
  v1_1x2_lines_a1          27  96->96   24545  split 1x2 lines                              1.7e-06 7.8e-07   1.4e-06 9.4e-07
  v2_2x4_lines_a1          27 192->192  13633  split 2x4 lines                              1.4e-06 1.0e-06   1.4e-06 1.2e-06
  v3_1x4_lines_a1          27 192->96   20449  split 1x4 lines                              1.7e-06 1.2e-06   1.6e-06 1.7e-06
  v4_1x8_lines_a1          27  32->32    4065  split 1x8 lines                              5.0e-07 5.1e-07   4.9e-07 5.9e-07
  v5_2x4_frag_a1           27  16->64   61409  split 2x4 frag                               5.6e-07 4.3e-07   7.6e-07 4.9e-07
  v6_1x4_frag_a1           27  48->48   40929  split 1x4 frag                               7.9e-07 6.2e-07   1.2e-06 6.6e-07
  v7_1x8_frag_a1           27 112->112  10209  split 1x8 frag                               1.0e-06 8.1e-07   1.4e-06 8.0e-07
  v8_1x16_frag_a1          27 112->112    993  split 1x16 frag                              5.9e-07 6.6e-07   6.4e-07 6.7e-07
  ksplit_lines_a1          27 128->96     141  split 1x4 lines, 9 x 3 offsets, combine      3.5e-07 6.7e-07   3.8e-07 6.2e-07
  ksplit_frag_a1           27  48->48     141  split 1x4 frag, 9 x 3 offsets, combine       3.5e-07 5.2e-07   3.0e-07 5.0e-07
  ksplit_odd_a1            27  96->192    141  split 1x4 lines, 5 x 6 offsets, combine      4.6e-07 5.1e-07   4.5e-07 4.6e-07
  ksplit_reduce_a1         27 128->96     141  split 1x4 lines, 9 x 3 offsets, reduce       3.5e-07 6.7e-07   3.8e-07 6.2e-07
  ksplit_odd_reduce_a1     27  96->192    141  split 1x4 lines, 5 x 6 offsets, reduce       4.6e-07 5.1e-07   4.5e-07 4.6e-07
  down_w2_a1                8  64->96   24545  split 1x2 lines                              1.0e-06 7.3e-07   9.7e-07 7.6e-07
  down_w8_a1                8  64->96    1345  split 1x8 lines                              5.1e-07 5.7e-07   4.8e-07 6.0e-07
  down_ksplit_a1            8  64->96     141  split 1x4 lines, 8 x 1 offsets, combine      2.5e-07 5.1e-07   2.4e-07 5.7e-07
  up_w2_a1                  8 128->96   24545  split 1x2 lines                              5.9e-07 8.8e-07   5.0e-07 9.3e-07
  up_w8_a1                  8 128->96    1345  split 1x8 lines                              2.0e-07 7.6e-07   3.1e-07 7.1e-07
  up_ksplit_a1              8 128->96     141  split 1x4 lines, 8 x 1 offsets, combine      1.7e-07 6.0e-07   2.0e-07 5.3e-07
  one_w2_a1                 1 320->160  14721  split 1x2 lines                              6.4e-07 1.6e-06   8.2e-07 1.6e-06
  one_w8_a1                 1 320->160    141  split 1x8 lines                              2.6e-07 8.5e-07   3.9e-07 7.8e-07
  v0_2x2_lines_a2          27  64->64   49121  bf16 2x2 lines                               7.8e-07 3.7e-07   7.7e-07 4.3e-07
  v1_1x2_lines_a2          27  96->96   24545  bf16 1x2 lines                               9.7e-07 4.6e-07   8.5e-07 5.2e-07
  v2_2x4_lines_a2          27 192->192  13633  bf16 2x4 lines                               1.0e-06 4.8e-07   8.2e-07 5.2e-07
  v3_1x4_lines_a2          27 192->96   27297  bf16 1x4 lines                               9.1e-07 5.1e-07   1.1e-06 6.9e-07
  v4_1x8_lines_a2          27  32->32    4065  bf16 1x8 lines                               2.5e-07 2.6e-07   3.6e-07 4.0e-07
  v5_2x4_frag_a2           27  16->64   81889  bf16 2x4 frag                                3.0e-07 3.3e-07   4.0e-07 4.1e-07
  v6_1x4_frag_a2           27  48->48   61409  bf16 1x4 frag                                4.9e-07 3.9e-07   5.2e-07 4.3e-07
  v7_1x8_frag_a2           27 112->112  15329  bf16 1x8 frag                                5.1e-07 4.4e-07   5.0e-07 5.1e-07
  v8_1x16_frag_a2          27 112->112    993  bf16 1x16 frag                               3.6e-07 3.2e-07   3.6e-07 3.1e-07
  ksplit_lines_a2          27 128->96     141  bf16 1x4 lines, 9 x 3 offsets, combine       2.0e-07 2.8e-07   2.2e-07 2.9e-07
  ksplit_frag_a2           27  48->48     141  bf16 1x4 frag, 9 x 3 offsets, combine        1.7e-07 2.1e-07   2.2e-07 2.2e-07
  ksplit_odd_a2            27  96->192    141  bf16 1x4 lines, 5 x 6 offsets, combine       2.1e-07 2.0e-07   2.2e-07 2.4e-07
  ksplit_reduce_a2         27 128->96     141  bf16 1x4 lines, 9 x 3 offsets, reduce        2.0e-07 2.8e-07   2.2e-07 2.9e-07
  ksplit_odd_reduce_a2     27  96->192    141  bf16 1x4 lines, 5 x 6 offsets, reduce        2.1e-07 2.0e-07   2.2e-07 2.4e-07
  down_w2_a2                8  64->96   24545  bf16 1x2 lines                               6.0e-07 3.5e-07   5.1e-07 4.2e-07
  down_w8_a2                8  64->96    1345  bf16 1x8 lines                               2.3e-07 2.8e-07   2.7e-07 3.8e-07
  down_ksplit_a2            8  64->96     141  bf16 1x4 lines, 8 x 1 offsets, combine       1.8e-07 2.0e-07   2.2e-07 2.8e-07
  up_w2_a2                  8 128->96   24545  bf16 1x2 lines                               2.2e-07 4.0e-07   2.6e-07 3.7e-07
  up_w8_a2                  8 128->96    1345  bf16 1x8 lines                               1.5e-07 3.3e-07   2.4e-07 3.8e-07
  up_ksplit_a2              8 128->96     141  bf16 1x4 lines, 8 x 1 offsets, combine       1.7e-07 2.9e-07   1.9e-07 2.1e-07
  one_w2_a2                 1 320->160  14721  bf16 1x2 lines                               2.9e-07 6.8e-07   4.5e-07 6.9e-07
  one_w8_a2                 1 320->160    141  bf16 1x8 lines                               1.2e-07 4.4e-07   1.9e-07 4.4e-07
  fp32_mfma                27  64->64    4065  fp32 1x4 frag                                1.1e-06 6.7e-07   1.2e-06 7.5e-07
  fp32_mfma_ksplit         27  96->192    161  fp32 1x4 frag, 7 x 4 offsets, combine        4.4e-07 5.3e-07   4.4e-07 6.8e-07
  fp32_mfma_ksplit_reduce  27  96->192    141  fp32 1x4 frag, 9 x 3 offsets, reduce         5.1e-07 5.1e-07   4.9e-07 4.6e-07
  fp32_mfma_down            8  32->64    4065  fp32 1x4 frag                                6.2e-07 4.4e-07   7.7e-07 4.8e-07
  tile_bpu1                27   6->128   8161  tile bpu 1                                   8.7e-07 3.2e-07   8.9e-07 3.7e-07
  tile_vec_bpu1            27  16->128   8161  tile bpu 1 vec                               1.1e-06 4.2e-07   1.3e-06 4.5e-07
  tile_bpu2                27   3->96   32737  tile bpu 2                                   5.8e-07 3.3e-07   6.0e-07 3.9e-07
  tile_vec_bpu2            27  16->96   32737  tile bpu 2 vec                               1.4e-06 3.9e-07   1.4e-06 4.8e-07
  tile_bpu3                27   6->128  32737  tile bpu 3                                   7.2e-07 3.3e-07   8.2e-07 4.5e-07
  tile_vec_bpu3            27  16->128  32737  tile bpu 3 vec                               1.2e-06 3.9e-07   1.4e-06 4.3e-07
  tile_bpu4                27   3->128  65505  tile bpu 4                                   6.5e-07 3.3e-07   6.6e-07 4.2e-07
  tile_vec_bpu4            27  16->128  65505  tile bpu 4 vec                               1.4e-06 4.0e-07   1.3e-06 4.7e-07
  tile_ksplit              27   6->32     141  tile bpu 1, 27 x 1 offsets, reduce           2.0e-07 2.0e-07   2.5e-07 2.5e-07
  scalar                   27  32->6     1000  scalar                                       1.7e-06 8.1e-07   1.5e-05 2.4e-05
"""
import functools
import json
import os
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref  # noqa: E402
from unet_train_ref import exact_voxels  # noqa: E402

from softgroup_amd.spconv import core  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MAX_ROWS = 200000
SPARE = 64                       # poisoned rows behind every output
MIN_ROWS = 141                   # no case below this: several tiles and a partial last one
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kind: 'subm' K = 27 | 'down' K = 8 strided | 'up' K = 8 inverse | 'one' K = 1
# want: what the query must report -- family; var = (nbw, wv, at) of a persistent variant; split = offsets split
# over several units; combine = in-launch combine; odd = k_per_split does not divide K; bpu / vec = tile kernel
# mode: plan = False -> no plan given; combine = 0 -> sg_spconv_set_combine(0)
Case = namedtuple('Case', 'name kind cin cout arith want mode')
KVOL = dict(subm=27, down=8, up=8, one=1)
FAMILY = {0: 'fp32', 1: 'split', 2: 'bf16'}


def _cases():
    out = []

    def add(name, kind, cin, cout, arith, mode=None, **want):
        out.append(Case(name, kind, cin, cout, arith, want, mode or {}))

    for ar in (1, 2):
        fam = FAMILY[ar]
        # the nine persistent variants on K = 27
        add(f'v0_2x2_lines_a{ar}', 'subm', 64, 64, ar, family=fam, var=(2, 2, 1), split=False)
        add(f'v1_1x2_lines_a{ar}', 'subm', 96, 96, ar, family=fam, var=(1, 2, 1), split=False)
        add(f'v2_2x4_lines_a{ar}', 'subm', 192, 192, ar, family=fam, var=(2, 4, 1), split=False)
        add(f'v3_1x4_lines_a{ar}', 'subm', 192, 96, ar, family=fam, var=(1, 4, 1), split=False)
        add(f'v4_1x8_lines_a{ar}', 'subm', 32, 32, ar, family=fam, var=(1, 8, 1), split=False)
        add(f'v5_2x4_frag_a{ar}', 'subm', 16, 64, ar, family=fam, var=(2, 4, 0), split=False)
        add(f'v6_1x4_frag_a{ar}', 'subm', 48, 48, ar, family=fam, var=(1, 4, 0), split=False)
        add(f'v7_1x8_frag_a{ar}', 'subm', 112, 112, ar, family=fam, var=(1, 8, 0), split=False)
        add(f'v8_1x16_frag_a{ar}', 'subm', 112, 112, ar, family=fam, var=(1, 16, 0), split=False)
        # offset-split layers: in-launch combine and the reduce kernel, k_per_split dividing K and not
        add(f'ksplit_lines_a{ar}', 'subm', 128, 96, ar, family=fam, var=(1, 4, 1), split=True, combine=1)
        add(f'ksplit_frag_a{ar}', 'subm', 48, 48, ar, family=fam, var=(1, 4, 0), split=True, combine=1)
        add(f'ksplit_odd_a{ar}', 'subm', 96, 192, ar, family=fam, var=(1, 4, 1), split=True, combine=1, odd=True)
        add(f'ksplit_reduce_a{ar}', 'subm', 128, 96, ar, dict(combine=0), family=fam, var=(1, 4, 1), split=True,
            combine=0)
        add(f'ksplit_odd_reduce_a{ar}', 'subm', 96, 192, ar, dict(combine=0), family=fam, var=(1, 4, 1), split=True,
            combine=0, odd=True)
        # K = 8 strided / inverse and the K = 1 shortcut: a two-wave variant, the 8-wave variant, the offset split
        # (K = 1 cannot split: ksplit <= K)
        for kind, cin, cout in (('down', 64, 96), ('up', 128, 96), ('one', 320, 160)):
            add(f'{kind}_w2_a{ar}', kind, cin, cout, ar, family=fam, wv=2, at=1, split=False)
            add(f'{kind}_w8_a{ar}', kind, cin, cout, ar, family=fam, var=(1, 8, 1), split=False)
            if kind != 'one':
                add(f'{kind}_ksplit_a{ar}', kind, cin, cout, ar, family=fam, var=(1, 4, 1), split=True, combine=1)
    add('fp32_mfma', 'subm', 64, 64, 0, family='fp32', split=False)
    add('fp32_mfma_ksplit', 'subm', 96, 192, 0, family='fp32', split=True, combine=1, odd=True)
    add('fp32_mfma_ksplit_reduce', 'subm', 96, 192, 0, dict(combine=0), family='fp32', split=True, combine=0)
    add('fp32_mfma_down', 'down', 32, 64, 0, family='fp32', split=False)
    for bpu, cout in ((1, 128), (2, 96), (3, 128), (4, 128)):       # (with 4 column blocks the kernel goes 1 -> 3 -> 4)
        add(f'tile_bpu{bpu}', 'subm', 6 if bpu % 2 else 3, cout, 1, family='tile', bpu=bpu, vec=0, split=False)
        add(f'tile_vec_bpu{bpu}', 'subm', 16, cout, 1, dict(plan=False), family='tile', bpu=bpu, vec=1, split=False)
    add('tile_ksplit', 'subm', 6, 32, 1, family='tile', bpu=1, vec=0, split=True, combine=0)
    add('scalar', 'subm', 32, 6, 1, dict(min_rows=1000), family='scalar')
    return out


CASES = _cases()


def _matches(info, want, K):
    if core.CONV_FAMILIES[info.family] != want['family']:
        return False
    if 'var' in want and (info.nbw, info.wv, info.at) != want['var']:
        return False
    for k in ('wv', 'at', 'vec', 'combine'):
        if k in want and getattr(info, k) != want[k]:
            return False
    if 'bpu' in want and info.blocks_per_unit != want['bpu']:
        return False
    if 'split' in want and (info.ksplit > 1) != want['split']:
        return False
    if want.get('odd') and K % info.k_per_split == 0:
        return False
    return True


def _rows_in_estimate(kind, m):
    return 4 * m if kind == 'down' else max(m // 3, 1) if kind == 'up' else m


def _query(case, m, cin, cout, rows_in=None):
    K = KVOL[case.kind]
    nin = _rows_in_estimate(case.kind, m) if rows_in is None else rows_in
    return core.conv_launch_info(m, nin, K, cin, cout, case.mode.get('plan', True), None, case.arith)


def _ok_rows(m):
    return m % 32 not in (0, 31)


def _smallest_rows(case, cin, cout):
    """smallest M_out <= MAX_ROWS, M_out % 32 not in {0, 31}, at which the query reports the case's form (None: none)"""
    hit = lambda m: _matches(_query(case, m, cin, cout), case.want, KVOL[case.kind])      # noqa: E731
    first = case.mode.get('min_rows', MIN_ROWS)
    grid = sorted({first} | {m for m in (int(1.03 ** i) for i in range(1, 420)) if first < m < MAX_ROWS} | {MAX_ROWS - 2})
    prev = first - 1
    for m in grid:
        if hit(m):
            lo, hi = prev, m                 # not at lo (or lo below the first size allowed), at hi
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (lo, mid) if hit(mid) else (mid, hi)
            m = hi
            while m <= MAX_ROWS and not (_ok_rows(m) and hit(m)):
                m += 1
            return m if m <= MAX_ROWS else None
        prev = m
    return None


@functools.lru_cache(maxsize=None)
def _alternatives(kind):
    """(Cin, Cout) of every layer of this kind in the channel lists of tests/golden/ref_configs.json"""
    with open(os.path.join(ROOT, 'tests', 'golden', 'ref_configs.json')) as f:
        cfgs = json.load(f)
    out = []
    for c, nb in sorted({(v['channels'], v['num_blocks']) for v in cfgs.values()}):
        planes = [c * (i + 1) for i in range(nb)]
        if kind in ('subm', 'one'):
            out += [(2 * p, p) for p in planes[:-1]] + ([(p, p) for p in planes] if kind == 'subm' else [])
        else:
            out += [(a, b) if kind == 'down' else (b, a) for a, b in zip(planes[:-1], planes[1:])]
    return out


def _extent(cells):
    """odd, unequal extents with at least `cells` cells"""
    e = max(int(round(cells ** (1 / 3))), 2)
    ext = [e + 3 | 1, e | 1, max(e - 2, 1) | 1]
    while ext[0] * ext[1] * ext[2] < cells:
        ext[0] += 2
    return ext


def _tables(kind, rows, rng):
    """oracle gather table with exactly `rows` output rows -> (table [rows, K], input rows)"""
    if kind == 'one':
        return conv_ref.identity_table(rows), rows
    if kind == 'subm':
        ext = _extent(rows / 0.3)                                   # ~8 of 27 neighbours present
        idx = exact_voxels(rng, rows, ext, 1)
        return conv_ref.subm_table(idx, ext), rows
    if kind == 'up':                                                # exactly one tap per row: even extents, no drop
        ext = [e + 1 for e in _extent(rows / 0.4)]
        idx = exact_voxels(rng, rows, ext, 1)
        _, up, m_parents = conv_ref.down_tables(idx, ext)
        assert ((up >= 0).sum(1) == 1).all()
        return up, m_parents
    # strided: `rows` parents, each with a random non-empty subset of its 8 children (dense-ish: 70 %)
    cext = _extent(rows / 0.5)
    parents = exact_voxels(rng, rows, cext, 1)
    keep = rng.random((rows, 8)) < 0.7
    keep[np.arange(rows), rng.integers(0, 8, rows)] = True
    p, k = np.nonzero(keep)
    fine = parents[p].copy()
    fine[:, 1:] = fine[:, 1:] * 2 + np.stack([k >> 2 & 1, k >> 1 & 1, k & 1], 1)
    fine = np.ascontiguousarray(fine[rng.permutation(len(fine))])
    child, _, m_out = conv_ref.down_tables(fine, [2 * e for e in cext])
    assert m_out == rows and len(fine) != rows
    return child, len(fine)


def _row_err(got, ref):
    scale = ref.abs().max(1, keepdim=True)[0].clamp(min=1e-300)
    return float(((got.double() - ref).abs() / scale).max())


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_layer_against_float64(case):
    from softgroup_amd import _lib as L
    lib = L.lib()
    K = KVOL[case.kind]
    torch.cuda.set_device(0)
    try:
        if 'combine' in case.mode:
            L.check(lib.sg_spconv_set_combine(case.mode['combine']), 'sg_spconv_set_combine')
        L.check(lib.sg_spconv_set_arithmetic(case.arith), 'sg_spconv_set_arithmetic')
        # ---- 1. the size at which the library says it runs this form
        rows = None
        for cin, cout in [(case.cin, case.cout)] + [s for s in _alternatives(case.kind) if s != (case.cin, case.cout)]:
            rows = _smallest_rows(case, cin, cout)
            if rows is not None:
                break
        assert rows is not None, f'no (Cin, Cout) reaches {case.want} with K = {K} below {MAX_ROWS} rows on this device'
        rng = np.random.default_rng(rows + cin)
        table, n_in = _tables(case.kind, rows, rng)
        info = _query(case, rows, cin, cout, rows_in=n_in)
        form = (core.CONV_FAMILIES[info.family], info.blocks_per_unit, info.vec, info.variant, info.nbw, info.wv, info.at,
                info.ksplit, info.k_per_split, info.combine, info.grid)
        assert _matches(info, case.want, K), f'{case.name}: K={K} {cin}->{cout} x {rows} rows runs {form}, not {case.want}'
        # ---- 2. the oracle's table, the library's plan over it
        g = torch.Generator(device=DEV).manual_seed(rows)
        nbr = torch.from_numpy(table).to(DEV).contiguous()
        plan = core._Plan(nbr, rows, K) if case.mode.get('plan', True) else None
        x = (torch.randn(n_in, cin, device=DEV, generator=g)
             * torch.exp(torch.empty(n_in, 1, device=DEV).uniform_(-7, 7, generator=g))).contiguous()
        w = torch.randn(cout, K, cin, device=DEV, generator=g) * 0.1
        res = torch.randn(rows, cout, device=DEV, generator=g)
        ps, pb = torch.rand(cout, device=DEV, generator=g) + 0.5, torch.randn(cout, device=DEV, generator=g) * 0.2
        as_, ab = torch.rand(cout, device=DEV, generator=g) + 0.5, torch.randn(cout, device=DEV, generator=g) * 0.2
        w_k8 = core.pack_weight(w, cout, K, cin, False)
        nb = lib.sg_spconv_conv_workspace_bytes(rows, cout)
        ws = L.workspace(nb, DEV) if nb > 256 else None
        xr, wr = (x.bfloat16(), w.bfloat16()) if case.arith == 2 and info.family == 4 else (x, w)
        line = []
        for epi in (False, True):
            # ---- 3. the call, into NaN-filled outputs with poisoned spare rows behind them
            out = torch.full((rows + SPARE, cout), float('nan'), device=DEV)
            out_act = torch.full((rows + SPARE, cout), float('nan'), device=DEV)
            ep = (L.ptr(ps), L.ptr(pb), L.ptr(res), L.ptr(as_), L.ptr(ab), L.ptr(out_act)) if epi else (None, ) * 6
            pl = (L.ptr(plan.order), L.ptr(plan.tile_mask), L.ptr(plan.nbr_tiles)) if plan is not None else (None, ) * 3
            L.check(lib.sg_spconv_gather_conv_f32(L.ptr(x), n_in, L.ptr(nbr), rows, K, cin, cout, L.ptr(w_k8), *ep, *pl,
                                                  L.ptr(out), L.ptr(ws), nb if ws is not None else 0, L.stream()),
                    'sg_spconv_gather_conv_f32')
            torch.cuda.synchronize()
            assert torch.isnan(out[rows:]).all() and torch.isnan(out_act[rows:]).all(), 'rows behind the output written'
            assert torch.isfinite(out[:rows]).all()
            assert torch.isfinite(out_act[:rows]).all() if epi else torch.isnan(out_act).all()
            # ---- 4. against the reference
            kw = dict(residual=res, post=(ps, pb), act=(as_, ab)) if epi else {}
            ref = conv_ref.layer(xr, wr, nbr, **kw)
            r32 = conv_ref.layer(xr, wr, nbr, dtype=torch.float32, bounds=False, **kw)
            pairs = [(out[:rows], ref.out, r32.out, ref.s_out, ref.ops_out)]
            if epi:
                pairs.append((out_act[:rows], ref.out_act, r32.out_act, ref.s_act, ref.ops_act))
            for got, want, want32, s_abs, ops in pairs:
                e32, err = _row_err(want32, want), _row_err(got, want)
                ceiling = (ref.n[:, None].double() + 8 + ops) * conv_ref.U32 * s_abs
                over = ((got.double() - want).abs() - ceiling).max().item()
                line.append((err, e32, over))
            del ref, r32
        print(f'{case.name:24s} K={K:2d} {cin:3d}->{cout:3d} x {rows:6d} rows  {form}  '
              + '  '.join(f'err {e:.2e} e32 {f:.2e}' for e, f, _ in line))
        for err, e32, over in line:
            assert over <= 0, f'{case.name}: {over:.3e} above the ceiling (n + 8 + ops) 2^-24 S_abs'
            assert err <= max(1e-5, 4 * e32), f'{case.name}: row error {err:.3e}, float32 reference {e32:.3e}'
    finally:
        lib.sg_spconv_set_arithmetic(-1)
        lib.sg_spconv_set_combine(-1)
