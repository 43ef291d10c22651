"""CPU side of the conv reference: tests/conv_ref.py against the CPU oracle, the dense-torch golden vectors and a
plain loop, and -- in the manner of tests/test_scale_thresholds.py -- the case list of tests/test_conv_ref_gpu.py
against the variant table and the thresholds in csrc/spconv_conv.hip: a variant added to or taken out of the
table, a new kernel family or a retuned constant fails here, before anyone goes to a GPU."""
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref  # noqa: E402
import test_conv_ref_gpu as G  # noqa: E402

import oracle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'softgroup_amd', 'csrc', 'spconv_conv.hip')


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---------------------------------------------------------------------------------------------------
# the helper itself
# ---------------------------------------------------------------------------------------------------
def test_reference_equals_the_oracle_conv_and_a_plain_loop():
    rng = np.random.default_rng(0)
    shape = [9, 7, 5]
    idx = G.exact_voxels(rng, 120, shape, 2)
    table = conv_ref.subm_table(idx, shape)
    x = rng.standard_normal((120, 5)).astype(np.float32)
    w = rng.standard_normal((12, 27, 5)).astype(np.float32)
    ref = conv_ref.layer(_t(x), _t(w), table)
    loop = conv_ref.dense_loop(x, w, table)
    np.testing.assert_allclose(ref.out.numpy(), loop, rtol=0, atol=1e-12)
    ora = oracle.subm_conv3d(x, table, w.reshape(12, 3, 3, 3, 5))
    np.testing.assert_allclose(ora, loop, rtol=1e-5, atol=1e-5)
    # S_abs and n: the same loop over absolute values; products = present taps x Cin
    np.testing.assert_allclose(ref.s_out.numpy(), conv_ref.dense_loop(np.abs(x), np.abs(w), table), rtol=0, atol=1e-12)
    assert np.array_equal(ref.n.numpy(), (table >= 0).sum(1) * 5)
    assert (ref.s_out.numpy() >= np.abs(ref.out.numpy())).all() and ref.out_act is None and ref.ops_out == 0
    # epilogues, written out
    res = rng.standard_normal((120, 12)).astype(np.float32)
    ps, pb, as_, ab = (rng.standard_normal(12).astype(np.float32) for _ in range(4))
    full = conv_ref.layer(_t(x), _t(w), table, residual=_t(res), post=(_t(ps), _t(pb)), act=(_t(as_), _t(ab)))
    out = np.maximum((loop + res) * ps.astype(np.float64) + pb, 0)
    np.testing.assert_allclose(full.out.numpy(), out, rtol=0, atol=1e-12)
    np.testing.assert_allclose(full.out_act.numpy(), np.maximum(out * as_.astype(np.float64) + ab, 0), rtol=0, atol=1e-12)
    assert (full.s_out.numpy() >= full.out.numpy()).all() and (full.s_act.numpy() >= full.out_act.numpy()).all()
    assert (full.ops_out, full.ops_act) == (3, 5)
    # float32 evaluation of the same thing: close, not equal; no bound quantities asked
    r32 = conv_ref.layer(_t(x), _t(w), table, dtype=torch.float32, bounds=False)
    assert r32.out.dtype == torch.float32 and r32.s_out is None
    err = np.abs(r32.out.double().numpy() - loop)
    assert 0 < err.max() and (err <= (ref.n.numpy()[:, None] + 1) * conv_ref.U32 * ref.s_out.numpy()).all()


def test_reference_equals_the_dense_torch_golden(golden):
    """K = 27, K = 8 strided and K = 8 inverse against torch.nn.functional's dense convolutions (fp32 golden)"""
    g = golden('sparse_conv_dense')
    idx, f, shape = g['indices'], g['feats'], [int(s) for s in g['shape']]
    cin, cout = f.shape[1], g['W_subm'].shape[0]
    sub = conv_ref.layer(_t(f), _t(g['W_subm'].reshape(cout, 27, cin)), conv_ref.subm_table(idx, shape))
    np.testing.assert_allclose(sub.out.numpy(), g['subm_out'], atol=2e-5, rtol=1e-5)
    child, up, m_out = conv_ref.down_tables(idx, shape)
    oi = oracle.down_rulebook(idx, shape)[0]
    dd = g['down_dense'][oi[:, 0], oi[:, 1], oi[:, 2], oi[:, 3]]
    down = conv_ref.layer(_t(f), _t(g['W_down'].reshape(cout, 8, cin)), child)
    assert m_out == len(oi) == down.out.shape[0]
    np.testing.assert_allclose(down.out.numpy(), dd, atol=2e-5, rtol=1e-5)
    # the inverse conv consumes the dense down output at the active rows; rows on the dropped last plane stay 0
    inv = conv_ref.layer(_t(dd), _t(g['W_inv'].reshape(cin, 8, cout)), up)
    np.testing.assert_allclose(inv.out.numpy(), g['inverse_out'], atol=2e-5, rtol=1e-5)
    assert ((up >= 0).sum(1) <= 1).all() and ((up >= 0).sum(1) == 0).any()
    one = conv_ref.layer(_t(f), _t(g['W_subm'].reshape(cout, 27, cin)[:, 13:14]), conv_ref.identity_table(len(f)))
    np.testing.assert_allclose(one.out.numpy(), f.astype(np.float64) @ g['W_subm'].reshape(cout, 27, cin)[:, 13].T.astype(np.float64),
                               rtol=0, atol=1e-12)


def test_table_builders_of_the_gpu_cases_give_exact_row_counts():
    rng = np.random.default_rng(1)
    for kind, rows in (('subm', 141), ('subm', 1001), ('down', 333), ('up', 777), ('one', 65)):
        table, n_in = G._tables(kind, rows, rng)
        assert table.shape == (rows, G.KVOL[kind]) and table.max() == n_in - 1 and table.min() >= -1
        if kind == 'down':
            assert n_in != rows and ((table >= 0).sum(1) >= 1).all() and ((table >= 0).sum(1) < 8).any()
            assert np.array_equal(np.sort(table[table >= 0]), np.arange(n_in))        # every fine row has one parent
        if kind == 'up':
            assert ((table >= 0).sum(1) == 1).all()
        if kind == 'subm':
            assert np.array_equal(table[:, 13], np.arange(rows)) and 3 < (table >= 0).sum(1).mean() < 14


# ---------------------------------------------------------------------------------------------------
# the case list against the source
# ---------------------------------------------------------------------------------------------------
def _source():
    with open(SRC) as f:
        return f.read()


def _const(src, name):
    m = re.search(r'constexpr\s+int\s+' + name + r'\s*=\s*(\d+)\s*;', src)
    assert m, f'constexpr int {name} not found'
    return int(m.group(1))


def _variants(src):
    """[(ck, nbw, wv, at)] of g_split_variants, in table order"""
    m = re.search(r'g_split_variants\[kSplitVariants\]\s*=\s*\{(.*?)\};', src, flags=re.S)
    assert m, 'the variant table not found'
    rows = re.findall(r'SG_SPLIT_VARIANT\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\)', m.group(1))
    assert re.search(r'#define SG_SPLIT_VARIANT\(CK, DEPTH, WPE, NBW, WV, AT\)', src)
    return [(int(ck), int(nbw), int(wv), int(at)) for ck, _, _, nbw, wv, at in rows]


def test_case_list_names_every_variant_and_family_in_the_source():
    src = _source()
    variants = _variants(src)
    assert len(variants) == _const(src, 'kSplitVariants') == 9, variants
    assert len(set(variants)) == len(variants)
    for ar in (1, 2):
        named = [c.want['var'] for c in G.CASES if c.arith == ar and 'var' in c.want and not c.want['split']
                 and c.kind == 'subm']
        assert sorted(named) == sorted((nbw, wv, at) for _, nbw, wv, at in variants), (ar, named)
    # line-wise variants work on 32-channel items, fragment-shaped ones on 16: the channels of each case fit its gather
    ck = {(nbw, wv, at): c for c, nbw, wv, at in variants}
    for c in G.CASES:
        if 'var' in c.want:
            assert c.cin % ck[c.want['var']] == 0 and (c.cin % 32 == 0) == (c.want['var'][2] == 1), c.name
            assert c.want['var'][0] == 1 or c.cout % 64 == 0, c.name
    # families: the enumeration of the launch decision, the names the binding gives them, the cases
    m = re.search(r'enum\s*\{([^}]*kFamScalar[^}]*)\}', src)
    assert m, 'the family enumeration not found'
    fams = re.findall(r'kFam(\w+)\s*=\s*(\d+)', m.group(1))
    assert [int(v) for _, v in fams] == list(range(len(fams)))
    assert [n.lower() for n, _ in fams] == [n.replace('bf16', 'b16') for n in G.core.CONV_FAMILIES]
    assert {c.want['family'] for c in G.CASES} == set(G.core.CONV_FAMILIES)
    # the general kernel: every blocks-per-unit instantiation, vectorised and not; both combine forms
    inst = sorted(int(b) for b in re.findall(r'launch_tile<(\d)>\(a,', src))
    assert inst == [1, 2, 3, 4]
    assert {(c.want['bpu'], c.want['vec']) for c in G.CASES if c.want['family'] == 'tile'} == {(b, v) for b in inst for v in (0, 1)}
    for fam in ('fp32', 'split', 'bf16'):
        assert {c.want.get('combine') for c in G.CASES if c.want['family'] == fam and c.want.get('split')} == {0, 1}, fam
        assert any(c.want.get('odd') for c in G.CASES if c.want['family'] == fam), fam
    # every kind of table on a two-wave variant, the 8-wave variant and (K > 1) the offset split, arithmetics 1 and 2
    for ar in (1, 2):
        for kind in ('down', 'up', 'one'):
            mine = [c for c in G.CASES if c.kind == kind and c.arith == ar]
            assert any(c.want.get('wv') == 2 for c in mine) and any(c.want.get('var') == (1, 8, 1) for c in mine), (ar, kind)
            assert kind == 'one' or any(c.want.get('split') for c in mine), (ar, kind)
    assert any((c.kind, c.cin, c.cout) == ('one', 320, 160) for c in G.CASES)


def test_case_shapes_sit_on_the_side_of_each_threshold_they_were_chosen_for():
    src = _source()
    tile = _const(src, 'kTileRows')
    assert tile == 32            # `M_out % 32 not in {0, 31}`: a partial last tile of more than one, fewer than 31 rows
    assert G._ok_rows(G.MIN_ROWS) and G.MIN_ROWS > 4 * tile and not G._ok_rows(64) and not G._ok_rows(63)
    m = re.search(r'w2_max\s*=\s*getenv\("SG_CONV_W2_MAX"\)\s*\?[^:]*:\s*(\d+)\s*;', src)
    assert m, 'w2_max not found'
    w2_max = int(m.group(1))
    assert re.search(r'use_w2\s*=[^;]*K \* \(Cin / 32\) <= w2_max', src)
    for c in G.CASES:
        if c.want.get('var', (0, 0, 0))[1] == 2 or c.want.get('wv') == 2:
            assert G.KVOL[c.kind] * (c.cin // 32) <= w2_max, c.name                 # two waves allowed
        if c.want.get('var') in ((2, 4, 1), (1, 4, 1)) and not c.want['split']:
            assert G.KVOL[c.kind] * (c.cin // 32) > w2_max, c.name                  # ... and ruled out
    for cin, cout in G._alternatives('down') + G._alternatives('up'):
        assert 8 * (cin // 32) <= w2_max                                           # K = 8 always qualifies
    m = re.search(r'const int target = target_env > 0 \? target_env : split \? (\d+) : (\d+);', src)
    assert m, 'the two targets of the offset split not found'
    t_split, t_other = int(m.group(1)), int(m.group(2))
    assert (t_split, t_other) == (1024, 2048)
    assert re.search(r'if \(waves < target / 2\)', src) and _const(src, 'kWavesPerWg') == 4
    tiles = (G.MIN_ROWS + tile - 1) // tile
    for c in G.CASES:
        if c.want.get('split'):                      # offsets are split at the smallest size a case may take
            persistent = c.want['family'] != 'tile'
            waves = tiles * ((c.cout + 31) // 32) * (4 if persistent else 1)
            assert waves < (t_split if c.want['family'] in ('split', 'bf16') else t_other) // 2, c.name
