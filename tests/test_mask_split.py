"""Masks cut into connected components: the numpy twin (``softgroup_amd.ops.split.mask_components_numpy``), the
list surface (``split_instances``) and the model wiring on the CPU path, against a brute force that builds the
O(m^2) adjacency matrix of every mask.  Equality everywhere; the reference has no such step.

The generators here are shared with tests/test_mask_split_gpu.py.  Lattice points are integer multiples of 0.25,
exact in float32: with ``radius = 0.25`` a pair one lattice step apart is at exactly the radius (adjacent) and a
diagonal pair at 0.3535 is not, so the lattice cases have 6-connectivity and their answers are written down by hand.
"""
import copy

import numpy as np
import pytest

from softgroup_amd.ops import split as MS
from softgroup_amd.util import rle_decode, rle_encode

R = 0.25


# ---- the brute-force definition --------------------------------------------------------------------------------
def brute(dense, xyz, radius, min_npoint=1, mode='split'):
    """dense bool [n, N] -> (rows bool [n_out, N], source [n_out], npoint [n_out]).  Per mask the full adjacency
    matrix by the rule, the minimum label over the neighbours (followed through the labels, which are members of
    the same component) until nothing changes, then the selection."""
    dense = np.asarray(dense, bool)
    n, N = dense.shape
    xyz = np.asarray(xyz, np.float32)
    r2 = float(radius) * float(radius)
    used = xyz[dense.any(0)].astype(np.float64)
    if not np.isfinite(used).all() or not (np.abs(np.floor(used / float(radius))) < 2.0 ** 31).all():
        raise ValueError('invalid coordinate of a mask point')
    rows, source, npoint = [], [], []
    for k in range(n):
        idx = np.flatnonzero(dense[k])
        m = idx.size
        if m == 0:
            continue
        X = xyz[idx].astype(np.float64)
        dx = X[:, None, 0] - X[None, :, 0]
        dy = X[:, None, 1] - X[None, :, 1]
        dz = X[:, None, 2] - X[None, :, 2]
        adj = (dx * dx + dy * dy) + dz * dz <= r2
        np.fill_diagonal(adj, True)
        lab = np.arange(m)
        while True:
            new = np.where(adj, lab[None, :], m).min(1)
            new = new[new]
            if np.array_equal(new, lab):
                break
            lab = new
        comps = [(int(r), int((lab == r).sum())) for r in np.flatnonzero(lab == np.arange(m))]
        if mode == 'largest':
            comps = [min(comps, key=lambda c: (-c[1], c[0]))]
        for r, size in comps:
            if size >= min_npoint:
                row = np.zeros(N, bool)
                row[idx[lab == r]] = True
                rows.append(row)
                source.append(k)
                npoint.append(size)
    return (np.array(rows, bool).reshape(len(rows), N), np.array(source, np.int32), np.array(npoint, np.int32))


def bits_of(dense):
    """dense bool [n, N] -> int32 bit rows [n, ceil(N / 32)]"""
    dense = np.asarray(dense, bool)
    n, N = dense.shape
    words = (N + 31) // 32
    out = np.zeros((n, words * 32), bool)
    out[:, :N] = dense
    if n == 0:
        return np.zeros((0, words), np.int32)
    return np.ascontiguousarray(np.packbits(out, axis=1, bitorder='little')).view(np.int32).reshape(n, words)


def dense_of(bits, N):
    bits = np.ascontiguousarray(bits)
    n = bits.shape[0]
    if n == 0:
        return np.zeros((0, N), bool)
    return np.unpackbits(bits.view(np.uint8).reshape(n, -1), axis=1, bitorder='little')[:, :N].astype(bool)


def same_as_brute(got, want, N):
    """got: (bit rows, source, npoint) of the code under test; want: brute()'s triple"""
    out_bits, source, npoint = (np.asarray(g) for g in got)
    rows, src, cnt = want
    words = (N + 31) // 32
    assert out_bits.shape == (len(src), words) and source.shape == (len(src), ) and npoint.shape == (len(src), )
    assert np.array_equal(source, src) and np.array_equal(npoint, cnt)
    assert np.array_equal(out_bits.view(np.int32), bits_of(rows))       # (the padding bits are zero)


# ---- hand-made cases ----------------------------------------------------------------------------------------------
def _lattice(cells):
    return (np.array(cells, np.float64) * R).astype(np.float32)


def _mask(N, *sets):
    m = np.zeros((len(sets), N), bool)
    for k, s in enumerate(sets):
        m[k, list(s)] = True
    return m


def _hand():
    """name -> dict(xyz, bits, N, radius, min_npoint, mode, want = [(source, [points])] or ValueError)"""
    cases = {}

    def add(name, xyz, dense, want, radius=R, min_npoint=1, mode='split', bits=None):
        xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
        cases[name] = dict(xyz=xyz, bits=bits_of(dense) if bits is None else bits, N=xyz.shape[0], radius=radius,
                           min_npoint=min_npoint, mode=mode, want=want)

    # two 2x2x2 blocks, the lattice plane x = 2 between them missing
    blocks = _lattice([(x, y, z) for x in (0, 1, 3, 4) for y in (0, 1) for z in (0, 1)])
    every = _mask(16, range(16))
    add('two_blocks', blocks, every, [(0, list(range(8))), (0, list(range(8, 16)))])
    add('min_npoint_drops_everything', blocks, every, [], min_npoint=9)
    add('largest_tie_takes_the_smaller_key', blocks, every, [(0, list(range(8)))], mode='largest')
    add('largest_takes_the_later_when_greater', blocks, _mask(16, list(range(5)) + list(range(8, 16))),
        [(0, list(range(8, 16)))], mode='largest')
    add('largest_below_min_npoint', blocks, every, [], mode='largest', min_npoint=9)
    # an L whose arms touch only diagonally
    add('l_shape_diagonal', _lattice([(0, 0, 0), (1, 0, 0), (2, 1, 0), (2, 2, 0)]), _mask(4, range(4)),
        [(0, [0, 1]), (0, [2, 3])])
    # a pair at exactly the radius; the same pair one float32 ulp further apart
    add('pair_at_radius', [(0, 0, 0), (R, 0, 0)], _mask(2, range(2)), [(0, [0, 1])])
    add('pair_one_ulp_beyond', [(0, 0, 0), (np.nextafter(np.float32(R), np.float32(1)), 0, 0)], _mask(2, range(2)),
        [(0, [0]), (0, [1])])
    # equal coordinates are adjacent
    add('duplicates', [(1, 1, 1), (5, 5, 5), (1, 1, 1), (1, 1, 1)], _mask(4, range(4)), [(0, [0, 2, 3]), (0, [1])])
    # negative coordinates: the cells left of 0 are floor's, not truncation's
    neg = [(-0.5, 0, 0), (-0.25, 0, 0), (0, 0, 0), (0.25, 0, 0), (-0.0625, 1, 0), (-0.3125, 1, 0),
           (0.1875, 1, 0), (-0.3125, -1, -0.3125), (-0.0625, -1, -0.0625)]      # (all exact in float32)
    add('negative_coordinates', neg, _mask(9, range(9)), [(0, [0, 1, 2, 3]), (0, [4, 5, 6]), (0, [7]), (0, [8])])
    # point 0 belongs to both masks; their other points are far apart
    shared = _lattice([(0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0), (0, 2, 0), (40, 0, 0)])
    add('shared_point', shared, _mask(6, [0, 1, 2, 5], [0, 3, 4]), [(0, [0, 1, 2]), (0, [5]), (1, [0, 3, 4])])
    add('empty_mask', shared, _mask(6, [], [0, 1, 5], []), [(1, [0, 1]), (1, [5])])
    cube = _lattice([(x, y, z) for x in range(3) for y in range(3) for z in range(3)])
    add('mask_of_every_point', cube, _mask(27, range(27)), [(0, list(range(27)))])
    beyond = bits_of(_mask(27, range(27)))
    beyond[:, -1] = -1                                      # bits 27 .. 31 set: ignored
    add('bits_beyond_n_ignored', cube, None, [(0, list(range(27)))], bits=beyond)
    add('no_masks', cube, np.zeros((0, 27), bool), [])
    nan = cube.copy()
    nan[13, 1] = np.nan
    add('nan_in_a_mask', nan, _mask(27, [12, 13, 14]), ValueError)
    add('nan_outside_every_mask', nan, _mask(27, [0, 1, 2], [26]), [(0, [0, 1, 2]), (1, [26])])
    inf = cube.copy()
    inf[3, 0] = np.inf
    add('inf_in_a_mask', inf, _mask(27, [3]), ValueError)
    far = cube.copy()
    far[3, 2] = 3.0e9                                       # finite, but cell 1.2e10 >= 2^31
    add('cell_out_of_range', far, _mask(27, [2, 3]), ValueError)
    return cases


HAND = _hand()


def check_hand(name, fn):
    """fn(bits, N, xyz, radius, min_npoint, mode) -> (out_bits, source, npoint) as numpy"""
    c = HAND[name]
    args = (c['bits'], c['N'], c['xyz'], c['radius'], c['min_npoint'], c['mode'])
    if c['want'] is ValueError:
        with pytest.raises(ValueError):
            fn(*args)
        return
    rows = _mask(c['N'], *[pts for _, pts in c['want']])
    want = (rows, np.array([s for s, _ in c['want']], np.int32), np.array([len(p) for _, p in c['want']], np.int32))
    same_as_brute(fn(*args), want, c['N'])


# ---- random clouds ------------------------------------------------------------------------------------------------
RADIUS = 0.1
# (n, N) -> seed; the large shapes are checked below to split at least a quarter of their masks and to leave at least
# a quarter whole
SHAPES = [(1, 31), (3, 33), (67, 2049), (300, 4097)]
CPU_SHAPES = [(40, 3000), (25, 1500), (12, 700)]


def random_case(n, N, seed=0, radius=RADIUS, neighbours=14.0):
    """Uniform points in a cube (centred on 0, so cells of both signs) with about ``neighbours`` points within the
    radius of each; a mask is the points inside 1 - 3 balls around random points, plus 0 - 3 stray points.
    -> (xyz float32 [N, 3], dense bool [n, N])"""
    rng = np.random.default_rng(1000 * seed + 7 * n + N)
    side = (N * (4.0 / 3.0) * np.pi * radius ** 3 / neighbours) ** (1.0 / 3.0)
    xyz = ((rng.random((N, 3)) - 0.5) * side).astype(np.float32)
    dense = np.zeros((n, N), bool)
    for k in range(n):
        for _ in range(int(rng.choice([1, 1, 1, 2, 3]))):
            c = xyz[rng.integers(N)].astype(np.float64)
            rho = rng.uniform(1.6, 2.6) * radius
            dense[k] |= ((xyz.astype(np.float64) - c) ** 2).sum(1) <= rho * rho
        if rng.random() < 0.5:
            dense[k, rng.integers(N, size=int(rng.integers(1, 4)))] = True
    return xyz, dense


_CACHE = {}


def reference(n, N, min_npoint=1, mode='split'):
    """the random case of a shape and the brute force's answer, computed once"""
    key = (n, N, min_npoint, mode)
    if key not in _CACHE:
        xyz, dense = random_case(n, N)
        _CACHE[key] = (xyz, dense, brute(dense, xyz, RADIUS, min_npoint, mode))
    return _CACHE[key]


def instance_list(dense, rle=True, seed=3):
    rng = np.random.default_rng(seed)
    n = dense.shape[0]
    return [dict(scan_id='scene0000_00', label_id=int(rng.integers(1, 19)), conf=float(np.float32(rng.random())),
                 pred_mask=rle_encode(dense[k].astype(np.int32)) if rle else dense[k].astype(np.int32))
            for k in range(n)]


def split_list_brute(insts, dense, xyz, radius, min_npoint, mode):
    rows, source, _ = brute(dense, xyz, radius, min_npoint, mode)
    return [dict(scan_id=insts[s]['scan_id'], label_id=insts[s]['label_id'], conf=insts[s]['conf'],
                 pred_mask=rle_encode(row.astype(np.int32))) for row, s in zip(rows, source)]


def same_lists(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert set(x) == set(y) == {'scan_id', 'label_id', 'conf', 'pred_mask'}
        assert x['scan_id'] == y['scan_id'] and x['label_id'] == y['label_id'] and x['conf'] == y['conf']
        assert x['pred_mask'] == y['pred_mask']


# ---- the numpy twin -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(HAND))
def test_twin_hand_made_cases(name):
    check_hand(name, MS.mask_components_numpy)


def test_brute_force_hand_made_cases():
    """the yardstick itself gives the answers written down by hand"""
    for name, c in HAND.items():
        if c['want'] is ValueError or name == 'bits_beyond_n_ignored':
            continue
        check_hand(name, lambda bits, N, xyz, r, mn, mode: (
            lambda t: (bits_of(t[0]), t[1], t[2]))(brute(dense_of(bits, N), xyz, r, mn, mode)))


@pytest.mark.parametrize('n,N', CPU_SHAPES + SHAPES)
def test_twin_equals_brute_force(n, N):
    xyz, dense, want = reference(n, N)
    if (n, N) in CPU_SHAPES:
        per_mask = np.bincount(want[1], minlength=n)
        assert 1 <= per_mask.min() and per_mask.max() <= 6, per_mask
        assert (per_mask > 1).mean() >= 0.25 and (per_mask == 1).mean() >= 0.25, per_mask
    same_as_brute(MS.mask_components_numpy(bits_of(dense), N, xyz, RADIUS), want, N)


@pytest.mark.parametrize('mode,min_npoint', [('largest', 1), ('split', 12), ('largest', 40)])
def test_twin_selection_equals_brute_force(mode, min_npoint):
    n, N = CPU_SHAPES[1]
    xyz, dense, want = reference(n, N, min_npoint, mode)
    assert 0 < len(want[1]) < len(reference(n, N)[2][1])
    same_as_brute(MS.mask_components_numpy(bits_of(dense), N, xyz, RADIUS, min_npoint, mode), want, N)


def test_twin_takes_packed_bytes_and_tensors():
    import torch
    n, N = CPU_SHAPES[2]
    xyz, dense, want = reference(n, N)
    bits = bits_of(dense)
    same_as_brute(MS.mask_components_numpy(bits.view(np.uint8), N, xyz, RADIUS), want, N)
    out = MS.mask_components(torch.from_numpy(bits), N, torch.from_numpy(xyz), RADIUS)
    assert all(torch.is_tensor(o) and o.dtype == torch.int32 for o in out)
    same_as_brute([o.numpy() for o in out], want, N)
    same_as_brute(MS.mask_components(bits, N, xyz, RADIUS), want, N)


def test_chain_is_one_component():
    """3000 collinear points one radius apart: far more links than any fixed number of propagation rounds"""
    xyz, dense = chain_case()
    out_bits, source, npoint = MS.mask_components_numpy(bits_of(dense), 3000, xyz, R)
    assert source.tolist() == [0] and npoint.tolist() == [3000]
    xyz, dense = chain_case(cut=1500)
    out_bits, source, npoint = MS.mask_components_numpy(bits_of(dense), 3000, xyz, R)
    assert source.tolist() == [0, 0] and npoint.tolist() == [1500, 1499]
    assert np.array_equal(dense_of(out_bits, 3000)[0], np.arange(3000) < 1500)


def chain_case(cut=None, shuffle=None):
    """one mask of 3000 collinear lattice points; ``cut``: that link's point is left out of the mask; ``shuffle``:
    a seed for the order in which the points are stored"""
    N = 3000
    pos = np.arange(N)
    if shuffle is not None:
        pos = np.random.default_rng(shuffle).permutation(N)
    xyz = np.zeros((N, 3), np.float32)
    xyz[:, 1] = (pos - 1000) * R                           # (exact in float32, both signs)
    dense = np.ones((1, N), bool)
    if cut is not None:
        dense[0, np.flatnonzero(pos == cut)] = False
    return xyz, dense


def test_argument_errors():
    xyz, dense = random_case(3, 33)
    bits = bits_of(dense)
    for bad in (0.0, -1.0, np.nan, np.inf, 1e200):
        with pytest.raises(ValueError):
            MS.mask_components_numpy(bits, 33, xyz, bad)
    with pytest.raises(ValueError):
        MS.mask_components_numpy(bits, 33, xyz, RADIUS, min_npoint=0)
    with pytest.raises(ValueError):
        MS.mask_components_numpy(bits, 33, xyz, RADIUS, mode='biggest')
    with pytest.raises(ValueError):
        MS.mask_components_numpy(bits, 33, xyz[:-1], RADIUS)


def test_split_params():
    assert MS.split_params(dict(radius=0.05)) == (0.05, 1, 'split')
    assert MS.split_params(dict(radius=1, min_npoint=50, mode='largest')) == (1.0, 50, 'largest')

    class Cfg:
        radius, min_npoint = 0.2, 7
    assert MS.split_params(Cfg()) == (0.2, 7, 'split')
    for bad in (dict(), dict(radius=0), dict(radius=0.1, min_npoint=0), dict(radius=0.1, min_npoint=2.5),
                dict(radius=0.1, mode='all'), dict(radius=float('nan'))):
        with pytest.raises(ValueError):
            MS.split_params(bad)


# ---- split_instances ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rle', [True, False], ids=['rle', 'dense'])
@pytest.mark.parametrize('mode,min_npoint', [('split', 1), ('split', 12), ('largest', 1)])
def test_split_instances_numpy(rle, mode, min_npoint):
    from softgroup_amd.util import split_instances
    n, N = CPU_SHAPES[1]
    xyz, dense, _ = reference(n, N)
    insts = instance_list(dense, rle)
    before = copy.deepcopy(insts)
    got = split_instances(insts, xyz, RADIUS, min_npoint, mode, backend='numpy')
    same_lists(got, split_list_brute(insts, dense, xyz, RADIUS, min_npoint, mode))
    assert all(g is not i for g in got for i in insts)
    for a, b in zip(insts, before):                         # inputs untouched
        assert a.keys() == b.keys() and a['conf'] == b['conf'] and a['label_id'] == b['label_id']
        assert np.array_equal(a['pred_mask'], b['pred_mask']) if not rle else a['pred_mask'] == b['pred_mask']
    for g in got:
        assert g['pred_mask'] == rle_encode(rle_decode(g['pred_mask']))


def test_split_instances_edge_cases():
    import torch

    from softgroup_amd.util import split_instances
    n, N = CPU_SHAPES[2]
    xyz, dense, _ = reference(n, N)
    insts = instance_list(dense)
    assert split_instances([], xyz, RADIUS) == []
    want = split_list_brute(insts, dense, xyz, RADIUS, 1, 'split')
    same_lists(split_instances(insts, torch.from_numpy(xyz), RADIUS, backend='numpy'), want)
    if not torch.cuda.is_available():
        same_lists(split_instances(insts, xyz, RADIUS), want)           # 'auto' without a GPU: numpy
    with pytest.raises(ValueError):
        split_instances(insts, xyz[:-1], RADIUS, backend='numpy')        # coordinates of another cloud
    with pytest.raises(ValueError):
        split_instances(insts, xyz, RADIUS, backend='gpu')
    # runs that are not ascending: numpy sorts them
    odd = [dict(scan_id='s', label_id=1, conf=0.5, pred_mask=dict(length=8, counts='7 2 1 2'))]
    pts = np.zeros((8, 3), np.float32)
    pts[:, 0] = np.arange(8)
    got = split_instances(odd, pts, 1.0, backend='numpy')
    assert [g['pred_mask']['counts'] for g in got] == ['1 2', '7 2']


# ---- the model, CPU path ------------------------------------------------------------------------------------------
def test_model_wiring_on_the_list_path():
    """``apply_split`` is what ``forward_test`` and ``ScanForward`` call on their finished list: absent / None returns
    the list itself, set it splits, and NMS -- when also set -- runs on the split list"""
    from softgroup_amd.util import nms_instances
    from softgroup_amd.util.split import apply_split
    n, N = CPU_SHAPES[1]
    xyz, dense, _ = reference(n, N)
    insts = instance_list(dense)
    assert apply_split(insts, xyz, None, None) is insts
    assert apply_split(insts, xyz, {}.get('split'), None) is insts
    cfg = dict(radius=RADIUS, min_npoint=5, mode='split')
    want = split_list_brute(insts, dense, xyz, RADIUS, 5, 'split')
    same_lists(apply_split(insts, xyz, cfg, None, backend='numpy'), want)
    nms = dict(thr=0.3, measure='min', class_agnostic=True)
    both = apply_split(insts, xyz, cfg, nms, backend='numpy')
    same_lists(both, nms_instances(want, 0.3, 'min', True, backend='numpy'))
    assert 0 < len(both) < len(want)
    with pytest.raises(ValueError):
        apply_split(insts, xyz, dict(radius=-1.0), None)
    with pytest.raises(AssertionError):
        apply_split(insts, xyz[:-1], cfg, None, backend='numpy')
