"""CPU side of the training convolution's reference: round_bf16, wgrad and input_grad of tests/conv_ref.py against
torch's own conversion, plain loops and float64 autograd; the case lists of tests/test_train_conv_ref_gpu.py
against csrc/spconv_train.hip (instantiations, clamps, targets, SG_WGRAD_CSPLIT, kRing -- a retuned constant or an
instantiation without a case fails here first) and through the two launch queries, which touch no device; and the
conditions the tables of the GPU cases were built for, as properties of the reference alone."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref  # noqa: E402
import test_train_conv_ref_gpu as T  # noqa: E402
from unet_train_ref import exact_voxels  # noqa: E402

from softgroup_amd.spconv import core  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'softgroup_amd', 'csrc', 'spconv_train.hip')
KVOL = T.KVOL


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---------------------------------------------------------------------------------------------------
# round_bf16
# ---------------------------------------------------------------------------------------------------
def _float_samples():
    rng = np.random.default_rng(0)
    bits = [rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)]
    hi = rng.integers(0, 2 ** 16, 20000, dtype=np.uint64).astype(np.uint32) << 16
    for low in (0x8000, 0x7FFF, 0x8001, 0x0000, 0xFFFF, 0x0001):      # ties and their neighbours, all exponents and signs
        bits.append(hi | np.uint32(low))
    bits.append(np.array(T.SPECIAL_BITS, np.uint32))
    bits.append(np.arange(0, 2 ** 17, dtype=np.uint32))                 # the smallest subnormals
    bits.append(np.arange(0x7F7F0000, 0x7F800000, 7, dtype=np.uint32))  # up to the largest finite value
    return torch.from_numpy(np.concatenate(bits).view(np.float32).copy())


def test_round_bf16_equals_torchs_conversion_bit_for_bit():
    x = _float_samples()
    got = conv_ref.round_bf16(x.double())
    want = x.bfloat16()
    nan = torch.isnan(x)
    assert nan.any() and torch.isnan(got[nan]).all()
    assert got.dtype == torch.float64
    g16 = got[~nan].float().bfloat16()
    assert torch.equal(g16.double(), got[~nan]), 'not on the bf16 grid'
    assert torch.equal(g16.view(torch.int16), want[~nan].view(torch.int16))          # signs of zero included
    # ties went to even, in both directions and for both signs
    for bits, even in ((0x3F808000, 0x3F80), (0x3F818000, 0x3F82), (0xBF808000, 0xBF80), (0xBF818000, 0xBF82)):
        v = torch.from_numpy(np.array([bits], np.uint32).view(np.float32).copy())
        r = conv_ref.round_bf16(v.double()).float().view(torch.int32)
        assert int(r) & 0xFFFFFFFF == even << 16


def test_round_bf16_rounds_once_and_is_monotone():
    # a double just above a bf16 midpoint that float32 rounds ONTO the midpoint: two roundings go to even (down)
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 3 * 2.0 ** -8 - 2.0 ** -40], dtype=torch.float64)
    twice = x.float().bfloat16().double()
    once = conv_ref.round_bf16(x)
    assert once.tolist() == [1.0 + 2.0 ** -7, 1.0 + 2.0 ** -7] and twice.tolist() == [1.0, 1.0 + 2.0 ** -6]
    rng = np.random.default_rng(1)
    v = np.concatenate([rng.standard_normal(100000) * np.exp(rng.uniform(-90, 88, 100000)),
                        _float_samples().double().numpy()])
    v = np.sort(v[np.isfinite(v)])
    r = conv_ref.round_bf16(torch.from_numpy(v)).numpy()
    assert (r[1:] >= r[:-1]).all() and np.isinf(r[0]) and np.isinf(r[-1])
    fin = np.isfinite(r)
    assert (np.abs(r[fin] - v[fin]) <= np.maximum(np.abs(v[fin]) * 2.0 ** -8, 2.0 ** -134)).all()


# ---------------------------------------------------------------------------------------------------
# wgrad and input_grad
# ---------------------------------------------------------------------------------------------------
def _small(kind, rng):
    if kind == 'subm':
        shape = [9, 7, 5]
        return conv_ref.subm_table(exact_voxels(rng, 120, shape, 2), shape), 120
    if kind == 'one':
        return conv_ref.identity_table(120), 120
    shape = [9, 7, 5] if kind == 'up' else [12, 10, 8]      # odd extents: the inverse table has rows without a tap
    idx = exact_voxels(rng, 120 if kind == 'up' else 400, shape, 1)
    child, up, m = conv_ref.down_tables(idx, shape)
    if kind == 'up':
        return up, m
    keep = np.sort(rng.choice(m, 120, replace=False))
    return child[keep], len(idx)


@pytest.mark.parametrize('kind', ['subm', 'down', 'up', 'one'])
def test_wgrad_and_input_grad_equal_plain_loops_and_autograd(kind):
    rng = np.random.default_rng(2)
    table, n_in = _small(kind, rng)
    assert table.shape == (120, KVOL[kind]) and (kind in ('subm', 'one') or (table < 0).any())
    cin, cout, K = 5, 6, table.shape[1]
    x = rng.standard_normal((n_in, cin)).astype(np.float32)
    g = rng.standard_normal((120, cout)).astype(np.float32)
    w = rng.standard_normal((cout, K, cin)).astype(np.float32)
    dw, s_w, n_w = conv_ref.wgrad(_t(x), _t(g), table)
    dx, s_x, n_x = conv_ref.input_grad(_t(g), _t(w), table, n_in)
    np.testing.assert_allclose(dw.numpy(), conv_ref.wgrad_loop(x, g, table), rtol=0, atol=1e-12)
    np.testing.assert_allclose(dx.numpy(), conv_ref.input_grad_loop(g, w, table, n_in), rtol=0, atol=1e-12)
    np.testing.assert_allclose(s_w.numpy(), conv_ref.wgrad_loop(np.abs(x), np.abs(g), table), rtol=0, atol=1e-12)
    np.testing.assert_allclose(s_x.numpy(), conv_ref.input_grad_loop(np.abs(g), np.abs(w), table, n_in), rtol=0, atol=1e-12)
    assert np.array_equal(n_w.numpy(), (table >= 0).sum(0))
    assert np.array_equal(n_x.numpy(), np.bincount(table[table >= 0], minlength=n_in) * cout)
    assert (s_w.numpy() >= np.abs(dw.numpy())).all() and (s_x.numpy() >= np.abs(dx.numpy())).all()
    # torch autograd of the forward reference, float64
    xt, wt = _t(x).double().requires_grad_(True), _t(w).double().requires_grad_(True)
    (conv_ref.layer(xt, wt, table, bounds=False).out * _t(g).double()).sum().backward()
    np.testing.assert_allclose(dx.numpy(), xt.grad.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(dw.numpy(), wt.grad.permute(1, 2, 0).numpy(), rtol=0, atol=1e-12)


# ---------------------------------------------------------------------------------------------------
# the case lists against the source
# ---------------------------------------------------------------------------------------------------
def _source():
    with open(SRC) as f:
        return f.read()


def _one(pattern, src, what):
    m = re.findall(pattern, src)
    assert len(m) == 1, f'{what}: {len(m)} matches of {pattern!r}'
    return m[0]


def _constants(src):
    c = {}
    c['kRing'] = int(_one(r'constexpr\s+int\s+kRing\s*=\s*(\d+)\s*;', src, 'kRing'))
    c['tile'] = int(_one(r'constexpr\s+int\s+kTRows\s*=\s*(\d+)\s*;', src, 'kTRows'))
    c['csplit'] = int(_one(r'#define SG_WGRAD_CSPLIT (\d+)', src, 'SG_WGRAD_CSPLIT'))
    c['rows_min'] = int(_one(r'if \(r < (\d+)\) r = \1;', src, 'the lower clamp of the chunk rows'))
    c['rows_max'] = int(_one(r'if \(r > (\d+)\) r = \1;', src, 'the upper clamp of the chunk rows'))
    c['wg_target'] = int(_one(r'chunks_want = \((\d+) \+ K \* w\.zs - 1\) / \(K \* w\.zs\)', src, 'the wgrad target'))
    lo, hi = _one(r'if \(waves < (\d+)\) \{\s*const long long want = \((\d+) \+ waves - 1\) / waves;', src,
                  'the wave target of the bf16 conv')
    assert lo == hi
    c['conv_target'] = int(lo)
    assert re.search(r'w\.csplit = \(K == 27 && r >= 64 \* SG_WGRAD_CSPLIT\) \? SG_WGRAD_CSPLIT : 1;', src)
    assert re.search(r'w\.v([io]) = \(C(in|out) % 2 == 0 && C(in|out) >= 64\) \? 2 : 1;', src)
    assert re.search(r'constexpr int wgrad_row_split\(int nst\) \{ return nst >= 3 \? 1 : \(nst == 2 \? 2 : 4\); \}', src)
    assert re.search(r'constexpr int kMaxPer = 8;\s*// chunk_rows <= 2048', src)
    return c


def _decide_conv(c, m, K, cin, cout, ws_bytes):
    nb = (cout + 31) // 32
    tiles = (m + c['tile'] - 1) // c['tile']
    cu = (nb + 3) // 4
    bpu = (nb + cu - 1) // cu
    ksplit, waves = 1, tiles * cu
    if waves < c['conv_target']:
        ksplit = min((c['conv_target'] + waves - 1) // waves, K)
        if ksplit > 1 and ws_bytes < ksplit * m * cout * 4:
            ksplit = 1
    kps = (K + ksplit - 1) // ksplit
    return (cu, bpu, int(cin % 16 == 0), (K + kps - 1) // kps, kps)


def _decide_wgrad(c, m, K, cin, cout):
    vi, vo = (2 if cin % 2 == 0 and cin >= 64 else 1), (2 if cout % 2 == 0 and cout >= 64 else 1)
    nst = ((cin + 32 * vi - 1) // (32 * vi)) * ((cout + 32 * vo - 1) // (32 * vo))
    zs = (nst + 3) // 4 if nst >= 3 else 1
    want = (c['wg_target'] + K * zs - 1) // (K * zs)
    r = ((m + want - 1) // want + 1) & ~1
    r = min(max(r, c['rows_min']), c['rows_max'])
    csplit = c['csplit'] if K == 27 and r >= 64 * c['csplit'] else 1
    return (vi, vo, nst, zs, r, (m + r - 1) // r, csplit, 1 if nst >= 3 else 2 if nst == 2 else 4)


def _full_ws(case):
    from softgroup_amd import _lib as L
    nb = L.lib().sg_spconv_conv_bf16_workspace_bytes(case.rows, case.cout)
    return nb if nb > 256 else 0


def test_constants_of_the_source_are_the_ones_the_cases_were_sized_for():
    c = _constants(_source())
    assert c == dict(kRing=3, tile=32, csplit=4, rows_min=128, rows_max=2048, wg_target=1024, conv_target=1024), c


def test_every_case_reaches_the_form_it_is_named_for():
    c = _constants(_source())
    for case in T.FCASES:
        K = KVOL[case.kind]
        for ws_bytes, want in ((_full_ws(case), case.want), (0, case.nows)):
            if want is None:
                continue
            info = core.conv_bf16_launch_info(case.rows, K, case.cin, case.cout, ws_bytes)
            assert T.form_f(info) == want, (case.name, T.form_f(info), want)
            assert _decide_conv(c, case.rows, K, case.cin, case.cout, ws_bytes) == want, case.name
            assert info.num_tiles == (case.rows + 31) // 32 and info.units == info.num_tiles * info.col_units * info.ksplit
            assert info.grid == (info.units + 3) // 4 and info.block == 256
            assert info.ws_used == (info.ksplit * case.rows * case.cout * 4 if info.ksplit > 1 else 0) <= ws_bytes
        # a partial last tile of more than one, fewer than 31 rows (12000 rows: the count the 3/3/2 split was named at)
        assert case.rows % 32 not in (0, 31) or case.name == 'down_split_332', case.name
    for case in T.WCASES:
        K = KVOL[case.kind]
        info = core.wgrad_launch_info(case.rows, K, case.cin, case.cout)
        assert T.form_w(info) == case.want, (case.name, T.form_w(info), case.want)
        assert _decide_wgrad(c, case.rows, K, case.cin, case.cout) == case.want, case.name
        from softgroup_amd import _lib as L
        assert (L.lib().sg_spconv_wgrad_workspace_bytes(case.rows, K, case.cin, case.cout)
                == info.chunks * info.csplit * K * case.cin * case.cout * 4 + 256)
    # the default workspace of the wrapper is the full one
    for case in T.FCASES:
        assert T.form_f(core.conv_bf16_launch_info(case.rows, KVOL[case.kind], case.cin, case.cout)) == case.want


def test_forward_cases_cover_every_instantiation_of_the_bf16_conv():
    src = _source()
    inst = sorted(int(b) for b in re.findall(r'launch_bf16<(\d)>\(a,', src))
    assert inst == [1, 2, 3, 4]
    assert len(re.findall(r'gather_conv_bf16_kernel<NBW, (?:true|false)><<<', src)) == 2
    forms = {(c.want[1], c.want[2]) for c in T.FCASES}
    assert forms == {(b, v) for b in inst for v in (0, 1)}, forms
    # split and unsplit, k_per_split dividing K and not, a last unit with fewer blocks, a partial last block
    assert {c.want[3] > 1 for c in T.FCASES} == {True, False}
    assert any(c.want[3] > 1 and KVOL[c.kind] % c.want[4] for c in T.FCASES)
    assert any(c.want[3] > 1 and KVOL[c.kind] % c.want[4] == 0 for c in T.FCASES)
    assert any(((c.cout + 31) // 32) % c.want[1] for c in T.FCASES) and any(c.cout % 32 for c in T.FCASES)
    assert any(c.nows is not None and c.nows[3] == 1 and c.want[3] > 1 for c in T.FCASES)        # the workspace rule
    assert {c.kind for c in T.FCASES} == {'subm', 'down', 'up', 'one'}
    # items per tile of the K = 1 cases: 1, 2 and 20 slices
    assert sorted((c.cin + 15) // 16 for c in T.FCASES if c.kind == 'one') == [1, 2, 20]
    # the modules: both gathers, forward and (channels swapped) backward
    assert {cin % 16 == 0 for _, cin, _ in T.MCASES} == {True, False} == {cout % 16 == 0 for _, _, cout in T.MCASES}
    assert {k for k, _, _ in T.MCASES} == {'subm', 'down', 'up'}


def test_wgrad_cases_cover_every_instantiation_and_size_class():
    src = _source()
    c = _constants(src)
    vecs = sorted((int(a), int(b)) for a, b in re.findall(r'conv_wgrad_kernel<TA, TG, (\d), (\d)><<<', src))
    types = sorted(re.findall(r'launch_wgrad<(\w+), (\w+)>\(in, g_out', src))
    assert vecs == [(1, 1), (1, 2), (2, 1), (2, 2)] and len(types) == 4
    name = {'uint16_t': 1, 'float': 0}
    inst = {(name[a], name[b], vi, vo) for a, b in types for vi, vo in vecs}
    assert len(inst) == 16
    covered = {(ta, tg, case.want[0], case.want[1]) for case in T.WCASES for ta, tg in case.types}
    assert covered == inst, inst - covered
    # every instantiation also on a meeting-free and on a meeting form where the shape allows: RS, zs, csplit, rows
    assert {case.want[7] for case in T.WCASES} == {1, 2, 4}
    for rs in (1, 2, 4):
        assert {t for case in T.WCASES if case.want[7] == rs for t in case.types} == set(T.ALL_TYPES), rs
    zs = {case.want[3] for case in T.WCASES}
    assert 1 in zs and max(zs) > 1 and {2, 3, 4} <= zs
    assert {case.want[6] for case in T.WCASES} == {1, c['csplit']}
    rows = {case.want[4] for case in T.WCASES}
    assert c['rows_min'] in rows and c['rows_max'] in rows and any(c['rows_min'] < r < c['rows_max'] for r in rows)
    assert c['rows_min'] + 2 in rows                                   # the first size above the clamp
    assert {KVOL[case.kind] for case in T.WCASES} == {27, 8, 1}
    assert any(case.want[6] > 1 and case.want[3] > 1 for case in T.WCASES)        # centre split with several z
    # more than 16 partial slots of an offset: the reduce's 16-step loop and its tail
    slots = [case.want[5] * case.want[6] for case in T.WCASES]
    assert any(s > 16 and s % 16 for s in slots) and any(s <= 4 for s in slots)
    assert any(case.want[5] > 16 and case.want[6] == 1 for case in T.WCASES)


# ---------------------------------------------------------------------------------------------------
# conditions on the reference alone
# ---------------------------------------------------------------------------------------------------
def _tile_masks(table):
    """[tiles, K] bool: tile t (32 consecutive rows) has a neighbour at offset k"""
    rows, K = table.shape
    pad = np.full(((rows + 31) // 32 * 32, K), -1, table.dtype)
    pad[:rows] = table
    return (pad.reshape(-1, 32, K) >= 0).any(1)


@pytest.mark.parametrize('case', [c for c in T.FCASES if c.flags], ids=lambda c: c.name)
def test_forward_tables_hold_what_they_were_built_for(case):
    c = _constants(_source())
    K = KVOL[case.kind]
    table, n_in = T.tables(case.name, case.kind, case.rows, case.density)
    assert table.shape == (case.rows, K) and table.max() == n_in - 1
    _, _, _, ksplit, kps = case.want
    present = _tile_masks(table)
    per_range = np.stack([present[:, lo:lo + kps].sum(1) for lo in range(0, K, kps)], 1)        # [tiles, ksplit]
    assert per_range.shape[1] == ksplit
    if 'empty_range' in case.flags:
        assert ksplit > 1 and (per_range == 0).any()
    if 'residues' in case.flags:
        n_slices = (case.cin + 15) // 16
        assert ksplit > 1 and set(np.unique(per_range * n_slices % c['kRing'])) == set(range(c['kRing']))
    if 'no_tap' in case.flags:
        taps = (table >= 0).sum(1)
        assert (taps == 0).any() and (taps <= 1).all()
        # ... also inside a tile that has rows with a tap, and not only in the last tile
        mixed = [(t[:32] == 0).any() and (t[:32] > 0).any() for t in np.array_split(taps, range(32, len(taps), 32))]
        assert sum(mixed) > 1


@pytest.mark.parametrize('case', [c for c in T.WCASES if c.flags], ids=lambda c: c.name)
def test_wgrad_tables_hold_what_they_were_built_for(case):
    K = KVOL[case.kind]
    table, _ = T.tables(case.name, case.kind, case.rows)
    rows, chunks, csplit = case.want[4], case.want[5], case.want[6]
    bounds = list(range(0, case.rows, rows))
    assert len(bounds) == chunks
    pairs = np.stack([(table[b:b + rows] >= 0).sum(0) for b in bounds])          # [chunks, K]
    if 'empty_pair' in case.flags:
        assert (pairs == 0).any()
    if 'odd' in case.flags:
        assert (pairs % 2 == 1).any()
    if 'single' in case.flags:
        assert (pairs == 1).any()
    if 'empty_piece' in case.flags:
        assert csplit > 1
        piece = (rows + csplit - 1) // csplit
        last = case.rows - bounds[-1]
        assert last - (csplit - 1) * piece <= 0 < last
