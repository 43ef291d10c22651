"""The shared index primitives above the sizes where they change form.

`exclusive_scan` (csrc/scan.h) and `radix_sort_pairs` (csrc/radix_sort.h) sit under every index product of the
library, and both -- with two of their callers -- take other code paths at sizes no other test reaches:

  scan        > kScanRawBlocks * kScanTile = 4 194 304 values: three launches, scan_block_sums_kernel's chunk loop
  radix sort  > 524 288 / 1 048 576 / 2 097 152 pairs: 16 / 32 / 64 keys per thread, 32 / 64 / 128 KB LDS tiles
              > 4 194 304 pairs: more than 256 workgroups, device-wide scan of the histogram, `totals == nullptr`
  pyramid     n_levels * M0 > 4 194 304: its position scan is a three-launch scan
  BFS         > kVisWords * 32 = 524 288 points: LOCAL replay of giant clusters without its LDS visited filter
              >= 2^21 points: giant clusters stay on the per-cluster kernel, claims in global memory

Every product is an integer and every comparison is exact.  The references are numpy in int64 (np.cumsum, a stable
np.argsort of keys built here) and the CPU oracle; nothing is compared with another run of the code under test
except where determinism itself is the property.  tests/test_scale_thresholds.py reads the constants out of the
sources and fails when one of the sizes below stops sitting on the side of its threshold it was chosen for.
"""
import os
import sys

import numpy as np
import pytest
import torch

import oracle
from softgroup_amd import _lib as L
from softgroup_amd import ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_spconv_gpu import HIST, _pyramid, _scene  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# ----------------------------------------------------------------------------------------------------------------
# the sizes (tests/test_scale_thresholds.py checks them against the constants in the sources)
SCAN_TILE = 2048
SCAN_SIZES = [0, 1, 2047, 2048, 2049, 524288, 4194303, 4194304, 4194305, 2304 * 2048, 2304 * 2048 + 1,
              4097 * 2048 + 5]
PLAN_SIZES = {27: [524288, 524289, 1048577, 2097153], 8: [2097153, 4194304, 4194305]}
PLAN_FAMILIES = ['uniform', 'constant', 'top', 'bottom']
PYRAMID_LEVELS = 7
PYRAMID_SCENE = dict(seed=4, n=900000, shape=[401, 399, 201], B=4)
BFS_N_NOVIS = 524289 + 3000         # (a): above the LDS visited filter, below the multi-workgroup replay's limit
BFS_N_PER_CLUSTER = 2097152 + 3000  # (b): giant clusters on the per-cluster kernel
BFS_SHEET, BFS_SLAB, BFS_CLIQUE = 150, 200, 300      # 22 500-point sheet, 40 000-point slab, 300-point cliques
OCTREE_N = 600000                   # tests/test_ops_gpu.py::test_octree_build_on_the_device_equals_the_host_export
SG_ERR_WORKSPACE = -2


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ----------------------------------------------------------------------------------------------------------------
# 1. exclusive_scan through sg_exclusive_scan_startlen
def scan_lengths(n, kind, seed=0):
    """int32 [n] in 0..3 with long runs of zeros (`runs`), or all ones (`ones`: position i must hold i)"""
    if kind == 'ones':
        return np.ones(n, np.int32)
    rng = np.random.default_rng(seed + n)
    v = rng.integers(0, 4, n).astype(np.int32)
    # zero runs of 1 .. 6000 values (several scan tiles, several 256-block chunks of block sums stay 0 at the big sizes)
    for s in rng.integers(0, max(n, 1), 40):
        v[s:s + int(rng.integers(1, 6000))] = 0
    if n > 3 * 256 * SCAN_TILE:
        v[256 * SCAN_TILE:2 * 256 * SCAN_TILE + 77] = 0      # one whole chunk of block sums (and a bit) is zero
    return v


def scan_reference(lengths):
    """(exclusive prefix, total) in int64"""
    c = np.cumsum(lengths.astype(np.int64))
    total = int(c[-1]) if len(c) else 0
    assert total < 2**31
    return c - lengths, total


@pytest.mark.parametrize('n', SCAN_SIZES)
def test_exclusive_scan_equals_cumsum(n):
    lib = L.lib()
    nb = lib.sg_scan_workspace_bytes(n)
    ws = torch.zeros(max(nb, 256), dtype=torch.uint8, device=DEV)
    for kind in ('runs', 'ones'):
        lengths = scan_lengths(n, kind)
        pre, total = scan_reference(lengths)
        sl_host = np.stack([np.full(n, -5, np.int32), lengths], 1) if n else np.zeros((0, 2), np.int32)
        outs = []
        for rep in range(2):                      # twice on the same workspace
            sl = t(sl_host) if n else torch.zeros((1, 2), dtype=torch.int32, device=DEV)
            meta = torch.full((2, ), -9, dtype=torch.int32, device=DEV)
            L.check(lib.sg_exclusive_scan_startlen(L.ptr(sl), n, L.ptr(meta), L.ptr(ws), nb, L.stream()),
                    'sg_exclusive_scan_startlen')
            got = sl.cpu().numpy()[:n]
            m = meta.cpu().numpy()
            assert int(m[0]) == total and int(m[1]) == -9, (kind, rep, m, total)
            assert np.array_equal(got[:, 1], lengths), (kind, rep)
            assert np.array_equal(got[:, 0].astype(np.int64), pre), (kind, rep)
            outs.append(got)
        assert np.array_equal(outs[0], outs[1])
    # a workspace one aligned unit (256 bytes) short: the workspace error, nothing written
    sl = t(sl_host) if n else torch.zeros((1, 2), dtype=torch.int32, device=DEV)
    before = sl.clone()
    meta = torch.full((2, ), -9, dtype=torch.int32, device=DEV)
    rc = lib.sg_exclusive_scan_startlen(L.ptr(sl), n, L.ptr(meta), L.ptr(ws), nb - 256, L.stream())
    torch.cuda.synchronize()
    assert rc == SG_ERR_WORKSPACE
    assert torch.equal(sl, before) and meta.tolist() == [-9, -9]


# ----------------------------------------------------------------------------------------------------------------
# 2. radix_sort_pairs through sg_spconv_plan on synthetic gather tables
def plan_masks(rows, K, family, seed=0):
    """uint32 [rows]: which of a row's K gather-table entries are present.
    The planner sorts by the mask with its bits permuted by offset frequency (most frequent offset = bit 0), so
      top     the low bits are set in every row (-> the key's low bits) and only the mask's top byte varies (K = 27:
              bits 24..26; K = 8: its top half): every pass but the last sees ONE digit, the last a few;
      bottom  only the bottom byte varies (K = 8: its bottom half), the rest is clear (-> the key's high bits):
              the first pass does all the work, later passes must keep its order;
      constant  every pass sees one digit for the whole tile (ranks across lanes, waves and rounds)."""
    rng = np.random.default_rng(seed + rows * 31 + K)
    full = (1 << K) - 1
    if family == 'constant':
        return np.full(rows, 0x5a5a5a5 & full | 1, np.uint32)
    lo_bits = list(range(8 if K > 8 else 4))
    hi_bits = list(range(24, K) if K > 8 else range(4, 8))
    vary = dict(uniform=list(range(K)), top=hi_bits, bottom=lo_bits)[family]
    m = np.zeros(rows, np.uint32)
    for j, k in enumerate(vary):       # distinct probabilities: the offset frequencies have no ties among them
        p = 0.15 + 0.7 * (j + 1) / (len(vary) + 1)
        m |= (rng.random(rows) < p).astype(np.uint32) << np.uint32(k)
    if family == 'top':
        m |= np.uint32((1 << hi_bits[0]) - 1)
    return m


def table_from_masks(mask, K):
    """int32 [rows + 1, K]: entry (r, k) = a row id if bit k of mask[r] is set, else -1; one all -1 row behind
    the table (what padding rows of a tile gather)"""
    rows = len(mask)
    r = np.arange(rows, dtype=np.int32)[:, None]          # (rows * 31 + 27 * 7919 < 2^31 at every size here)
    k = np.arange(K, dtype=np.int32)[None, :]
    val = (r * np.int32(31) + k * np.int32(7919)) % np.int32(max(rows, 1))
    nbr = np.full((rows + 1, K), -1, np.int32)
    nbr[:rows] = np.where((mask[:, None] >> np.arange(K, dtype=np.uint32)) & 1, val, -1)
    return nbr


def popcount32(x):
    return np.unpackbits(np.ascontiguousarray(x, np.uint32).view(np.uint8).reshape(-1, 4), axis=1).sum(1, dtype=np.int64)


def plan_reference_order(mask, K):
    """the planner's row sequence, independently: key = mask bits permuted by offset frequency (rarest offset =
    most significant, ties: lower offset more common), rows ascending by key, equal keys in ascending row order"""
    m = mask.astype(np.int64)
    freq = np.array([int(((m >> k) & 1).sum()) for k in range(K)], np.int64)
    pos = np.array([sum(1 for o in range(K) if freq[o] > freq[k] or (freq[o] == freq[k] and o < k))
                    for k in range(K)])
    key = np.zeros(len(m), np.int64)
    for k in range(K):
        key |= ((m >> k) & 1) << int(pos[k])
    return np.argsort(key, kind='stable')


def check_plan(order, tmask, ntiles, nbr_ext, K, mask=None):
    """order [T*32], tmask [T + HIST], ntiles [T*32*K] (numpy, from the device) against the table nbr_ext
    [rows + 1, K] (last row all -1)"""
    rows = len(nbr_ext) - 1
    T = (rows + 31) // 32
    order = order[:T * 32].reshape(T, 32)
    valid = order >= 0
    assert valid.sum() == rows and np.array_equal(np.bincount(order[valid], minlength=rows), np.ones(rows, np.int64))
    if mask is None:
        mask = ((nbr_ext[:rows] >= 0).astype(np.uint32) << np.arange(K, dtype=np.uint32)).sum(1, dtype=np.uint32)
    ref_order = plan_reference_order(mask, K)
    # the set of tiles: 32 consecutive rows of the stable sequence each, -1 behind the last row
    ref = np.full(T * 32, -1, np.int64)
    ref[:rows] = ref_order
    ref = ref.reshape(T, 32)
    assert (order[:, 0] >= 0).all()
    assert np.array_equal(order[np.argsort(order[:, 0])], ref[np.argsort(ref[:, 0])])
    # tile masks, heaviest first, histogram of the weights behind the masks
    row_mask = np.where(valid, mask[np.clip(order, 0, None)], 0).astype(np.uint32)
    tm = tmask[:T].view(np.uint32)
    assert np.array_equal(tm, np.bitwise_or.reduce(row_mask, 1))
    pop = popcount32(tm)
    assert (np.diff(pop) <= 0).all()
    hist = tmask[T:T + HIST].view(np.uint32)
    assert np.array_equal(hist[:33], np.bincount(pop, minlength=33)) and (hist[33:] == 0).all()
    # the tile-major copy of the table
    exp = nbr_ext[np.where(valid, order, rows).reshape(-1)]
    assert np.array_equal(ntiles[:T * 32 * K].reshape(T * 32, K), exp)


def _run_plan(nbr_ext, K):
    lib = L.lib()
    rows = len(nbr_ext) - 1
    T = (rows + 31) // 32
    nbr = t(nbr_ext[:rows])
    order = torch.full((T * 32, ), -99, dtype=torch.int32, device=DEV)
    tmask = torch.full((T + HIST, ), -99, dtype=torch.int32, device=DEV)
    ntiles = torch.full((T * 32 * K, ), -99, dtype=torch.int32, device=DEV)
    nb = lib.sg_spconv_plan_workspace_bytes(rows)
    ws = L.workspace(nb, DEV)
    L.check(lib.sg_spconv_plan(L.ptr(nbr), rows, K, L.ptr(order), L.ptr(tmask), L.ptr(ntiles), L.ptr(ws), nb,
                               L.stream()), 'sg_spconv_plan')
    torch.cuda.synchronize()
    return order.cpu().numpy(), tmask.cpu().numpy(), ntiles.cpu().numpy()


@pytest.mark.parametrize('family', PLAN_FAMILIES)
@pytest.mark.parametrize('K,rows', [(K, r) for K in (27, 8) for r in PLAN_SIZES[K]])
def test_plan_sort_is_stable_at_every_tile_size(K, rows, family):
    mask = plan_masks(rows, K, family)
    nbr_ext = table_from_masks(mask, K)
    order, tmask, ntiles = _run_plan(nbr_ext, K)
    check_plan(order, tmask, ntiles, nbr_ext, K, mask)


# ----------------------------------------------------------------------------------------------------------------
# 3. the whole-pyramid index build at a training-batch size
def pyramid_scene():
    p = PYRAMID_SCENE
    return _scene(np.random.default_rng(p['seed']), p['n'], p['shape'], B=p['B']), list(p['shape'])


def test_whole_pyramid_index_build_at_a_training_batch_size():
    """7 levels over a batch of 4 crops (odd extents: a plane is dropped at every level): the position scan of
    sg_spconv_pyramid_rows runs over n_levels * M0 values -- above 4 194 304, its three-launch form -- and the wide
    sort over all levels' rows with 32 keys per thread.  Row counts, coordinates, SubM / strided / inverse tables
    bit-exact against the oracle's per-level chain; every plan against the independent stable reference."""
    idx, shape = pyramid_scene()
    n_levels = PYRAMID_LEVELS
    M0 = len(idx)
    assert M0 * n_levels > 4194304, M0
    rows, lv = _pyramid(idx, shape, n_levels)
    cur, sh = idx, list(shape)

    def ext(tab):
        return np.concatenate([tab, np.full((1, tab.shape[1]), -1, np.int32)])

    def plan_of(p):
        return tuple(x.cpu().numpy() for x in p)

    for l in range(n_levels):
        d = lv[l]
        assert rows[l] == len(cur) and len(cur) > 0, (l, rows, len(cur))
        assert np.array_equal(d['indices'].cpu().numpy()[:len(cur) * 4].reshape(-1, 4), cur)
        nbr = oracle.subm_rulebook(cur, sh)
        assert np.array_equal(d['nbr'].cpu().numpy()[:len(cur) * 27].reshape(-1, 27), nbr)
        check_plan(*plan_of(d['subm']), ext(nbr), 27)
        if l + 1 == n_levels:
            break
        oi, in2out, child, osh = oracle.down_rulebook(cur, sh)
        assert np.array_equal(d['in2out'].cpu().numpy()[:len(cur)], in2out)
        assert np.array_equal(d['child'].cpu().numpy()[:len(oi) * 8].reshape(-1, 8), child)
        k = (cur[:, 1] & 1) * 4 + (cur[:, 2] & 1) * 2 + (cur[:, 3] & 1)
        inv = np.full((len(cur), 8), -1, np.int32)
        inv[np.arange(len(cur)), k] = in2out
        assert np.array_equal(d['inv'].cpu().numpy()[:len(cur) * 8].reshape(-1, 8), inv)
        check_plan(*plan_of(d['down']), ext(child), 8)
        check_plan(*plan_of(d['up']), ext(inv), 8)
        cur, sh = oi, osh


# ----------------------------------------------------------------------------------------------------------------
# 4. BFS above the two point-count gates, on hand-built CSR graphs
def _lattice_edges(w, h, offsets):
    """(src, dst) of a w x h lattice, node = x * h + y, one edge per in-range offset"""
    x, y = np.meshgrid(np.arange(w), np.arange(h), indexing='ij')
    x, y = x.reshape(-1), y.reshape(-1)
    src, dst = [], []
    for dx, dy in offsets:
        ok = (x + dx >= 0) & (x + dx < w) & (y + dy >= 0) & (y + dy < h)
        src.append((x * h + y)[ok])
        dst.append(((x + dx) * h + (y + dy))[ok])
    return np.concatenate(src), np.concatenate(dst)


def bfs_graph(n, seed=0):
    """CSR neighbour lists (ascending, symmetric, self included) over n points: one 150 x 150 sheet with
    4-neighbour lists, one 200 x 200 slab whose lists hold the 15 x 15 lattice window (64 .. 225 entries:
    fat levels), four 300-point cliques, every other point alone; ids scattered by a random permutation.
    -> idx int32 [E], start_len int32 [n, 2], component of every point (0 sheet, 1 slab, 2..5 cliques, -1 alone)"""
    rng = np.random.default_rng(seed + n)
    perm = rng.permutation(n).astype(np.int64)
    src, dst, comp = [], [], np.full(n, -1, np.int32)
    base = 0
    s, d = _lattice_edges(BFS_SHEET, BFS_SHEET, [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)])
    src.append(s + base), dst.append(d + base)
    comp[perm[base:base + BFS_SHEET**2]] = 0
    base += BFS_SHEET**2
    win = [(dx, dy) for dx in range(-7, 8) for dy in range(-7, 8)]
    s, d = _lattice_edges(BFS_SLAB, BFS_SLAB, win)
    src.append(s + base), dst.append(d + base)
    comp[perm[base:base + BFS_SLAB**2]] = 1
    base += BFS_SLAB**2
    for c in range(4):
        a = np.arange(BFS_CLIQUE)
        src.append(np.repeat(a, BFS_CLIQUE) + base), dst.append(np.tile(a, BFS_CLIQUE) + base)
        comp[perm[base:base + BFS_CLIQUE]] = 2 + c
        base += BFS_CLIQUE
    assert base < n
    rest = np.arange(base, n)
    src.append(rest), dst.append(rest)
    key = np.sort(perm[np.concatenate(src)] * n + perm[np.concatenate(dst)])
    idx = (key % n).astype(np.int32)
    lens = np.bincount(key // n, minlength=n).astype(np.int64)
    start_len = np.stack([np.cumsum(lens) - lens, lens], 1).astype(np.int32)
    return idx, start_len, comp


BFS_SIZES = sorted([BFS_CLIQUE] * 4 + [BFS_SHEET**2, BFS_SLAB**2])
_bfs_cache = {}


def _bfs_case(n):
    """graph + oracle result (threshold 2.0: the points that are alone are dropped), computed once per size"""
    if n not in _bfs_cache:
        _bfs_cache.clear()           # (one size at a time: the big one is 100 MB)
        idx, sl, comp = bfs_graph(n)
        mean = np.array([-1.0], np.float32)
        rci, rco = oracle.bfs_cluster(mean, idx, sl, 2.0, 0)
        assert sorted(np.diff(rco).tolist()) == BFS_SIZES         # the giants ARE there
        assert int(sl[:, 1].min()) >= 1 and int(sl[comp == 1, 1].min()) >= 60
        _bfs_cache[n] = (idx, sl, comp, rci, rco, t(idx), t(sl))
    return _bfs_cache[n]


@pytest.mark.parametrize('env', [{}, {'SG_BFS_BIG_LOCAL': '0'}, {'SG_BFS_BIG_LOCAL': '1', 'SG_BFS_FORCE_FALLBACK': '2'},
                                 {'SG_BFS_BIG_LOCAL': '1', 'SG_BFS_FORCE_FALLBACK': '3'}],
                         ids=['default', 'no-local', 'local-gave-up', 'both-gave-up'])
def test_bfs_above_the_visited_filter(env, monkeypatch):
    """527 289 points: the default replay of the two giant clusters is the LOCAL form WITHOUT its LDS visited
    filter (no hook set); then the forms behind it, as test_bfs_cluster_bigger_than_the_lds_claim_array runs them"""
    idx, sl, comp, rci, rco, d_idx, d_sl = _bfs_case(BFS_N_NOVIS)
    for k in ('SG_BFS_BIG_LOCAL', 'SG_BFS_FORCE_FALLBACK', 'SG_BFS_BIG_LOCAL_NOVIS', 'SG_BFS_BIG_FAST',
              'SG_BFS_BIG_LOCAL_WGS', 'SG_BFS_BIG_LOCAL_EVERY'):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ci, co = ops.bfs_cluster(torch.tensor([-1.0]), d_idx, d_sl, 2.0, 0)
    assert np.array_equal(co.cpu().numpy(), rco)
    assert np.array_equal(ci.cpu().numpy(), rci)          # membership AND member order


def test_bfs_segments_above_the_visited_filter():
    """two segment ids with their own thresholds on the same graph: segment 0 (sheet, two cliques) keeps clusters
    of >= 301 points, segment 1 (slab, two cliques) of >= 2; clusters come in the order of their seeds"""
    idx, sl, comp, rci, rco, d_idx, d_sl = _bfs_case(BFS_N_NOVIS)
    n = len(sl)
    rng = np.random.default_rng(5)
    seg = np.where(comp >= 0, comp & 1, rng.integers(0, 2, n)).astype(np.int32)
    thr = np.array([301.0, 2.0], np.float32)
    ci, co = ops.bfs_cluster_segments(d_idx, d_sl, t(thr), t(seg))
    sizes = np.diff(rco)
    seeds = rci[rco[:-1], 1]
    keep = sizes >= thr[seg[seeds]]
    assert sorted(sizes[keep].tolist()) == [BFS_CLIQUE, BFS_CLIQUE, BFS_SHEET**2, BFS_SLAB**2]
    exp_off = np.concatenate([[0], np.cumsum(sizes[keep])]).astype(np.int32)
    rows = np.repeat(keep, sizes)
    exp_idx = rci[rows].copy()
    exp_idx[:, 0] = np.repeat(np.arange(int(keep.sum()), dtype=np.int32), sizes[keep])
    assert np.array_equal(co.cpu().numpy(), exp_off)
    assert np.array_equal(ci.cpu().numpy(), exp_idx)


def test_bfs_giants_on_the_per_cluster_kernel():
    """2 100 152 points (>= 2^21): the 22 500- and the 40 000-point cluster are replayed by the per-cluster kernel
    itself, claims in the global owner array"""
    idx, sl, comp, rci, rco, d_idx, d_sl = _bfs_case(BFS_N_PER_CLUSTER)
    ci, co = ops.bfs_cluster(torch.tensor([-1.0]), d_idx, d_sl, 2.0, 0)
    assert np.array_equal(co.cpu().numpy(), rco)
    assert np.array_equal(ci.cpu().numpy(), rci)
    _bfs_cache.clear()
