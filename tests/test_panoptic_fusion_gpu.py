"""sg_panoptic_fusion (csrc/instances.hip) against tests/panoptic_ref.py on every form of its walker: the five
widths of panoptic_walk_kernel<SPL>, the listed and the per-lane word walk, a swap of the order registers, a
second trip of the decisions-to-ids scan, the division branch of the skip threshold, the dense kernel on the
rows it exists for, and both grid-stride loops past their block caps.  The operation is exact: every
comparison is assert_array_equal.

Every case: a random visiting order that is no identity, labels 1 + k % 251 (a rank / instance mix-up shows
in the class), cls_offset 10, semantic_classes 19, thing_class_min 11, random semantic classes; the workspace
has exactly sg_panoptic_fusion_workspace_bytes and is followed by 4 KiB of a pattern, and so is `out`; both
guards must survive.  Wherever the row fits the sparse walk the case runs a second time under
SG_PANOPTIC_DENSE=1.

The cases and what they have to reach are built and checked WITHOUT a GPU (the builders below touch no device;
tests/test_panoptic_ref.py runs `conditions` on every one of them): outside the threshold and degenerate
cases every 64-rank order block and every 2048-rank scan trip of the reference holds a pasted and a skipped
instance (a trailing group of fewer than 8 ranks: one of either)."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import panoptic_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 4096
WS_FILL, OUT_FILL = 0xA5, 0x5A5A5A5A

WALK_SIZES = [65536, 65537, 131073, 262145, 524289, 1048576, 1048577]
WALK_WIDTH = {65536: 1, 65537: 2, 131073: 4, 262145: 8, 524289: 16, 1048576: 16, 1048577: None}
WALK_SEED = {}                                  # (seeds: chosen on the host so that the reference meets `conditions`)
ORDER_BLOCK_COUNTS = [1, 63, 64, 65, 128, 129, 200]
ORDER_BLOCK_SEED = {65: 4, 129: 3}
ID_SCAN_COUNTS = [2048, 2049, 4100]
ID_SCAN_SEED = {2048: 0, 2049: 6, 4100: 0}
LIST_ORDERS = ['large_first', 'interleaved']
THRESHOLDS = ['below', 'at', 'above', 'zero', 'one', 'div7of13', 'div5of13']
TINY_ROWS = [1, 31, 32, 33]
MANY = 65535
LARGE = ('X', 'Y', 'Z')


# ---------------------------------------------------------------------------------------------------
# cases (host only)
# ---------------------------------------------------------------------------------------------------
def _order(rng, n_inst):
    order = rng.permutation(n_inst).astype(np.int32)
    while n_inst > 1 and np.array_equal(order, np.arange(n_inst)):
        order = rng.permutation(n_inst).astype(np.int32)
    return order


def _case(name, rng, n, points_of, order, skip_iou=0.5, **extra):
    n_inst = len(points_of)
    labels = P.labels_for(n_inst)
    sem = rng.integers(0, P.SEMANTIC_CLASSES, n).astype(np.int64)
    ref = P.panoptic_ref(points_of, order, labels, sem, n, P.CLS_OFFSET, skip_iou, P.SEMANTIC_CLASSES,
                         P.THING_CLASS_MIN)
    return SimpleNamespace(name=name, n=n, n_inst=n_inst, points_of=points_of, order=np.asarray(order, np.int32),
                           labels=labels, sem=sem, skip_iou=skip_iou, ref=ref, bits=P.pack_bits(points_of, n), **extra)


@functools.lru_cache(maxsize=None)
def walk_case(n):
    rng = np.random.default_rng([1, n, WALK_SEED.get(n, 0)])
    order = _order(rng, 70)
    points_of, kinds, copy_of = P.mixed_masks(rng, n, 70, order)
    return _case(f'walk{n}', rng, n, points_of, order, kinds=kinds, copy_of=copy_of)


@functools.lru_cache(maxsize=None)
def order_block_case(n_inst):
    rng = np.random.default_rng([2, n_inst, ORDER_BLOCK_SEED.get(n_inst, 0)])
    order = _order(rng, n_inst)
    points_of, kinds, copy_of = P.mixed_masks(rng, 2000, n_inst, order)
    return _case(f'order{n_inst}', rng, 2000, points_of, order, kinds=kinds, copy_of=copy_of)


def _windowed_order(rng, n_inst, window=32):
    """a random permutation that keeps neighbours close: the windows of 32 consecutive instances in a random
    order, each shuffled inside.  (Instance k of the id-scan case only ever overlaps k - 1 and k + 1; under a
    uniform permutation of thousands both are too rarely visited within the same 64 ranks for every order
    block to hold a skip.)"""
    starts = rng.permutation(np.arange(0, n_inst, window))
    order = np.concatenate([a + rng.permutation(min(window, n_inst - a)) for a in starts]).astype(np.int32)
    assert np.array_equal(np.sort(order), np.arange(n_inst)) and not np.array_equal(order, np.arange(n_inst))
    return order


@functools.lru_cache(maxsize=None)
def id_scan_case(n_inst):
    rng = np.random.default_rng([3, n_inst, ID_SCAN_SEED[n_inst]])
    return _case(f'scan{n_inst}', rng, 3 * n_inst, P.id_scan_masks(n_inst), _windowed_order(rng, n_inst))


@functools.lru_cache(maxsize=None)
def many_case():
    rng = np.random.default_rng([4, MANY])
    order = _order(rng, MANY)
    return _case('many', rng, 2048, P.many_instance_masks(rng, order), order)


@functools.lru_cache(maxsize=None)
def list_case(which):
    rng = np.random.default_rng([5, 300000])              # the same masks for both orders
    points_of, ix = P.list_boundary_masks(rng)
    if which == 'large_first':
        names = ['Z', 'X', 'Y', 'x_last', 'x_tail', 'r1', 'y_head', 'y_first', 'x_head', 'r2', 'y_tail', 'y_last',
                 'x_first', 'r0']
    else:               # (r0 is a run that ends on the row's last point: it would take y_last's point before Y)
        names = ['r1', 'x_first', 'X', 'x_head', 'r2', 'x_last', 'y_last', 'Y', 'y_tail', 'x_tail', 'y_first',
                 'y_head', 'Z', 'r0']
    order = np.array([ix[s] for s in names], np.int32)
    assert sorted(order.tolist()) == list(range(len(points_of))) and not np.array_equal(order, np.arange(len(order)))
    return _case(f'list_{which}', rng, 300000, points_of, order, ix=ix, names=names)


def threshold_overlap(which):
    """overlap and size of the instance on the threshold: 37 of 111, and two pairs found by a search over
    sizes below 200 for which the sign of ti - fl(skip_iou * den) and the quotient ti / den decide differently"""
    return {'div7of13': (7, 13), 'div5of13': (5, 13)}.get(which, (37, 111))


def threshold_value(which):
    ti, tc = threshold_overlap(which)
    s = ti / (tc + 1e-5)
    return {'below': float(np.nextafter(s, 0.0)), 'at': s, 'above': float(np.nextafter(s, 1.0)), 'zero': 0.0,
            'one': 1.0, 'div7of13': s, 'div5of13': float(np.nextafter(s, 0.0))}[which]


@functools.lru_cache(maxsize=None)
def threshold_case(which):
    rng = np.random.default_rng([6])
    points_of, order, names = P.threshold_masks(*threshold_overlap(which))
    return _case(f'threshold_{which}', rng, 400, points_of, order, skip_iou=threshold_value(which), names=names)


@functools.lru_cache(maxsize=None)
def tiny_case(n):
    rng = np.random.default_rng([7, n])
    order = _order(rng, 6)
    points_of, kinds, copy_of = P.mixed_masks(rng, n, 6, order)
    return _case(f'tiny{n}', rng, n, points_of, order, kinds=kinds, copy_of=copy_of)


def _kinds_present(c):
    return sorted(set(int(k) for k in c.kinds))


def conditions(c):
    """what the case was built to reach, asserted on the reference alone"""
    if c.name.startswith(('walk', 'order', 'scan', 'many', 'list')):
        assert P.block_problems(c.ref.stats, P.ORDER_BLOCK) == [], c.name
        assert P.block_problems(c.ref.stats, P.SCAN_TRIP) == [], c.name
    assert c.ref.n_ids == int(c.ref.pasted.sum()) and len(c.ref.pasted) == c.n_inst
    words = P.words_of(c.n)
    if c.name.startswith('walk'):
        n = c.n
        assert _kinds_present(c) == [P.RUN, P.SCATTER, P.COPY, P.ENDS, P.TAIL]
        if WALK_WIDTH[n] is None:
            assert words > P.TAKEN_WORDS and P.walk_width(n) is None      # the dense kernel, with no knob set
            assert P.words_of(n - 1) == P.TAKEN_WORDS
        else:
            assert words <= P.TAKEN_WORDS and P.walk_width(n) == WALK_WIDTH[n]
            # the first size of a width: one point less takes the width before it
            if n & 1:
                assert P.walk_width(n - 1) < P.walk_width(n)
        # 70 x padded words is more than panoptic_summary_kernel's 4096 x 256 threads from n = 524 289 on;
        # 70 x words is more than panoptic_assign_kernel's 8192 x 256 threads at n = 1 048 576 (at 524 289 it
        # is 1 146 950 of 2 097 152: that loop is passed once): both grid-stride loops go round a second time
        assert (70 * P.summary_words_of(n) * 32 > P.SUMMARY_CAP) == (n >= 524289)
        assert (70 * words > P.ASSIGN_CAP) == (n >= 1048576)
        # a scattered instance with a non-zero word under every summary word j of a lane (words 2048 j ...)
        scattered = [k for k in range(c.n_inst) if c.kinds[k] == P.SCATTER]
        groups = [(c.bits[scattered, lo:lo + 2048] != 0).any(axis=1) for lo in range(0, words, 2048)]
        assert np.all(groups, axis=0).any(), 'a scattered row under every j'
        # a run lies under ONE summary word, the row's last bit is used
        for k in range(c.n_inst):
            if c.kinds[k] == P.RUN:
                assert len(set((c.points_of[k] >> 10).tolist())) == 1
        assert (c.bits[:, words - 1] >> np.uint32((n - 1) & 31) & 1).any()
        st = c.ref.stats.sum(0)
        assert st[P.PASTED_FREE] and st[P.PASTED_OVERLAP] and st[P.SKIPPED] >= 10
        # every 65 536-point stretch (the summary word j of every lane) decides a copy: skipped, and pasted
        # once its points in that stretch are left out
        rank_of = np.argsort(c.order)
        decided = set()
        for k, (_, g) in c.copy_of.items():
            if g in decided or c.ref.pasted[rank_of[k]]:
                continue
            without = list(c.points_of)
            without[k] = c.points_of[k][(c.points_of[k] >> 16) != g]
            if P.panoptic_ref(without, c.order, c.labels, c.sem, n, P.CLS_OFFSET, c.skip_iou, P.SEMANTIC_CLASSES,
                              P.THING_CLASS_MIN).pasted[rank_of[k]]:
                decided.add(g)
        assert decided == set(range((n + 65535) // 65536)), sorted(decided)
    if c.name.startswith('order'):
        assert (c.n_inst - 1) // 64 == {1: 0, 63: 0, 64: 0, 65: 1, 128: 1, 129: 2, 200: 3}[c.n_inst]   # order swaps
        if c.n_inst >= 5:
            assert _kinds_present(c) == [P.RUN, P.SCATTER, P.COPY, P.ENDS, P.TAIL]
        if c.n_inst in (65, 129):
            # the one rank behind a swap: pasted, with points of its own -- its instance shows in the output
            assert c.ref.pasted[-1] and (c.ref.out >> 16 == c.ref.n_ids).any()
    if c.name.startswith('scan'):
        trips = (c.n_inst + P.SCAN_TRIP - 1) // P.SCAN_TRIP
        assert trips == {2048: 1, 2049: 2, 4100: 3}[c.n_inst]
        first_trip = int(c.ref.pasted[:P.SCAN_TRIP].sum())
        assert first_trip > 0                                  # the second trip's `base`
        if c.n_inst == 2049:
            # one rank in the second trip: pasted, so that base + 1 is an id in the output (more than 2048 ids
            # AND a skip at a rank >= 2048 cannot both be had from 2049 instances)
            assert c.ref.pasted[2048] and c.ref.n_ids == first_trip + 1
        if c.n_inst == 4100:
            assert c.ref.n_ids > 2048
            assert (~c.ref.pasted[2048:]).any() and c.ref.pasted[2048:4096].any() and c.ref.pasted[4096:].any()
            assert int(c.ref.out.max() >> 16) == c.ref.n_ids
    if c.name == 'many':
        assert c.n_inst == 65535 and words == 64
        assert c.ref.pasted[63488:].any()                      # the last word of `pasted`
        assert c.ref.stats[:, P.PASTED_FREE].sum() and c.ref.stats[:, P.PASTED_OVERLAP].sum()
    if c.name.startswith('list'):
        assert P.walk_width(c.n) == 8 and words == 9375
        nz = (c.bits != 0).sum(axis=1)
        assert nz[c.ix['X']] == P.LIST_CAP and nz[c.ix['Y']] == P.LIST_CAP + 1 and nz[c.ix['Z']] == words
        assert len(c.points_of[c.ix['X']]) == P.LIST_CAP and len(c.points_of[c.ix['Z']]) == c.n
        assert (nz[[v for s, v in c.ix.items() if s not in LARGE]] <= 1000).all() and len(c.ix) == 14
        rank = {s: c.names.index(s) for s in c.names}
        large = {s: bool(c.ref.pasted[rank[s]]) for s in LARGE}
        assert large == (dict(X=False, Y=False, Z=True) if c.name.endswith('large_first') else dict(X=True, Y=True, Z=True))
        # ordinary instances that are skipped BECAUSE of a pasted large one: pasted when the large ones are left out
        small_order = np.array([c.ix[s] for s in c.names if s not in LARGE], np.int32)
        alone = P.panoptic_ref(c.points_of, small_order, c.labels, c.sem, c.n, P.CLS_OFFSET, c.skip_iou,
                               P.SEMANTIC_CLASSES, P.THING_CLASS_MIN)
        small_names = [s for s in c.names if s not in LARGE]
        due = [s for i, s in enumerate(small_names) if alone.pasted[i] and not c.ref.pasted[rank[s]]]
        if c.name.endswith('large_first'):
            assert len(due) == len(small_names)              # all of them: Z took every point
        else:
            # the probes of X and Y that are visited after it and before Z: skipped because of X (Y)
            probes = [s for s in small_names if s[0] in 'xy' and rank[s.upper()[0]] < rank[s] < rank['Z']]
            assert set(probes) == {'x_head', 'x_last', 'x_tail', 'y_tail', 'y_first', 'y_head'} <= set(due)
            # ... and the two that are visited before it are pasted: X (Y) is then pasted WITH overlap
            assert c.ref.pasted[rank['x_first']] and c.ref.pasted[rank['y_last']]
            assert c.ref.stats[rank['X'], P.PASTED_OVERLAP] and c.ref.stats[rank['Y'], P.PASTED_OVERLAP]
    if c.name.startswith('threshold'):
        which = c.name.split('_')[1]
        decided = dict(zip(c.names, c.ref.pasted.tolist()))
        ti, tc = threshold_overlap(which)
        den = tc + 1e-5
        if which in ('below', 'at', 'above', 'div7of13', 'div5of13'):
            assert abs(ti - c.skip_iou * den) <= 1e-9 * den             # the division decides, not the sign
            assert decided == dict(A=True, B=True, C=which not in ('below', 'div5of13'), D=True, E=True, F=False, G=True)
            if which.startswith('div'):                                 # ... and the sign would decide otherwise
                assert (not (ti - c.skip_iou * den > 0.0)) != decided['C']
        elif which == 'zero':
            assert decided == dict(A=True, B=True, C=False, D=True, E=True, F=False, G=False)
        else:
            assert decided == dict(A=True, B=True, C=True, D=True, E=True, F=True, G=True)
            assert c.ref.n_ids == 7 and int(c.ref.out.max() >> 16) == 7 and not (c.ref.out >> 16 == 6).any()
        # the empty row D consumed an id: E, visited right after it, is two ids above the instance before D
        e_id = int(c.ref.out[300] >> 16)
        assert e_id == int(c.ref.pasted[:4].sum()) + 1 and not (c.ref.out >> 16 == e_id - 1).any()


ALL_CASES = ([(walk_case, n) for n in WALK_SIZES] + [(order_block_case, k) for k in ORDER_BLOCK_COUNTS] +
             [(id_scan_case, k) for k in ID_SCAN_COUNTS] + [(list_case, w) for w in LIST_ORDERS] +
             [(threshold_case, w) for w in THRESHOLDS] + [(tiny_case, n) for n in TINY_ROWS] + [(many_case,)])


# ---------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fuse(n_inst, n, bits, order, labels, sem, skip_iou, expect_error=False):
    """one call of sg_panoptic_fusion with guarded buffers; bits / order / labels may be None (null pointers)"""
    from softgroup_amd import _lib as L
    lib = L.lib()
    nb = int(lib.sg_panoptic_fusion_workspace_bytes(n_inst, n))
    ws = torch.full((nb + GUARD,), WS_FILL, dtype=torch.uint8, device='cuda')
    out = torch.full((n + GUARD // 4,), OUT_FILL, dtype=torch.int32, device='cuda')
    sem_d = _dev(sem) if n else torch.zeros(1, dtype=torch.int64, device='cuda')
    hold = [None if a is None else _dev(a) for a in (None if bits is None else bits.view(np.int32), order, labels)]
    rc = lib.sg_panoptic_fusion(L.ptr(hold[0]), n_inst, n, L.ptr(hold[1]), L.ptr(hold[2]), L.ptr(sem_d), P.CLS_OFFSET,
                                float(skip_iou), P.SEMANTIC_CLASSES, P.THING_CLASS_MIN, L.ptr(out), L.ptr(ws), nb,
                                L.stream())
    torch.cuda.synchronize()
    if expect_error:
        with pytest.raises(L.SoftGroupHipError, match='sg_panoptic_fusion'):
            L.check(rc, 'sg_panoptic_fusion')
        assert bool((out == OUT_FILL).all()), '`out` must be untouched'
    else:
        L.check(rc, 'sg_panoptic_fusion')
    assert bool((ws[nb:] == WS_FILL).all()), 'written behind the workspace'
    assert bool((out[n:] == OUT_FILL).all()), 'written behind `out`'
    return out[:n].cpu().numpy().view(np.uint32)


def check_case(c, monkeypatch):
    conditions(c)
    monkeypatch.delenv('SG_PANOPTIC_DENSE', raising=False)
    got = fuse(c.n_inst, c.n, c.bits, c.order, c.labels, c.sem, c.skip_iou)
    np.testing.assert_array_equal(got, c.ref.out, err_msg=f'{c.name}: default path')
    if P.words_of(c.n) <= P.TAKEN_WORDS:
        monkeypatch.setenv('SG_PANOPTIC_DENSE', '1')
        dense = fuse(c.n_inst, c.n, c.bits, c.order, c.labels, c.sem, c.skip_iou)
        np.testing.assert_array_equal(dense, c.ref.out, err_msg=f'{c.name}: dense walk')


@pytest.mark.parametrize('n', WALK_SIZES)
def test_every_walk_width_and_the_dense_fallback(n, monkeypatch):
    """the last size of SPL 1, the first sizes of SPL 2, 4, 8 and 16, the last sparse size and the first row
    that takes the dense kernel with no knob set; from 524 289 points on the summary kernel, at 1 048 576 the
    assign kernel as well, loops past its block cap"""
    check_case(walk_case(n), monkeypatch)


@pytest.mark.parametrize('which', LIST_ORDERS)
def test_list_boundary(which, monkeypatch):
    """8192 non-zero words (the last listed row), 8193 (the first one walked per lane) and a row with every
    point, visited first (Z pasted; X and Y compared and skipped) and interleaved after small instances (X and
    Y pasted: the small instances made of their first and last words are skipped because of them)"""
    check_case(list_case(which), monkeypatch)


@pytest.mark.parametrize('n_inst', ORDER_BLOCK_COUNTS)
def test_order_blocks(n_inst, monkeypatch):
    """0, 1, 2 and 3 swaps of the order registers, with the instance counts around a swap; the one rank behind
    the swap (65, 129) is pasted with points of its own.  (A single instance is pasted: that case has no skip.)"""
    check_case(order_block_case(n_inst), monkeypatch)


@pytest.mark.parametrize('n_inst', ID_SCAN_COUNTS)
def test_id_scan_trips(n_inst, monkeypatch):
    """one, two and three trips of the decisions-to-ids scan; the later trips start from a non-zero base.
    4100 instances give more than 2048 ids and skip at ranks >= 2048.  2049 instances cannot do both (more than
    2048 ids of 2049 means no skip at all): there rank 2048, alone in the second trip, is pasted, so that its id,
    base + 1, is in the output.  The order is random inside windows of 32 instances and over the windows: an
    instance only ever overlaps its neighbours, and a uniform permutation leaves early order blocks without a skip."""
    check_case(id_scan_case(n_inst), monkeypatch)


def test_largest_instance_count(monkeypatch):
    """65 535 instances: every word of `pasted` is used, the last id has 16 bits"""
    check_case(many_case(), monkeypatch)


def test_one_instance_too_many_is_an_error():
    n_inst, n = 65536, 2048
    fuse(n_inst, n, np.zeros((n_inst, 64), np.uint32), np.arange(n_inst, dtype=np.int32)[::-1].copy(),
         P.labels_for(n_inst), np.zeros(n, np.int64), 0.5, expect_error=True)


@pytest.mark.parametrize('which', THRESHOLDS)
def test_skip_threshold(which, monkeypatch):
    """overlap 37 of 111 against skip_iou one ulp below, at and one ulp above 37 / (111 + 1e-5): |ti - skip den|
    is within 1e-9 den, the double division decides, and only the value below skips; skip_iou 0 (any overlap
    skips, none pastes) and 1 (a fully taken instance is pasted and uses an id without a point); an all-zero
    row uses an id as well"""
    check_case(threshold_case(which), monkeypatch)


def test_no_instances(monkeypatch):
    """null bits, order and labels, as native_scan._panoptic passes them: sem, unclaimed thing classes -> 19"""
    rng = np.random.default_rng(8)
    for n in (1, 777):
        sem = rng.integers(0, P.SEMANTIC_CLASSES, n).astype(np.int64)
        if n > 1:
            assert (sem >= P.THING_CLASS_MIN).any() and (sem < P.THING_CLASS_MIN).any()
        want = np.where(sem >= P.THING_CLASS_MIN, P.SEMANTIC_CLASSES, sem).astype(np.uint32)
        ref = P.panoptic_ref([], np.zeros(0, np.int32), np.zeros(0, np.int32), sem, n, P.CLS_OFFSET, 0.5,
                             P.SEMANTIC_CLASSES, P.THING_CLASS_MIN)
        np.testing.assert_array_equal(ref.out, want)
        for dense in (False, True):
            if dense:
                monkeypatch.setenv('SG_PANOPTIC_DENSE', '1')
            else:
                monkeypatch.delenv('SG_PANOPTIC_DENSE', raising=False)
            np.testing.assert_array_equal(fuse(0, n, None, None, None, sem, 0.5), want)


def test_no_points():
    got = fuse(3, 0, np.zeros((3, 0), np.uint32), np.array([2, 0, 1], np.int32), P.labels_for(3), np.zeros(0, np.int64), 0.5)
    assert got.size == 0
    assert fuse(0, 0, None, None, None, np.zeros(0, np.int64), 0.5).size == 0


@pytest.mark.parametrize('n', TINY_ROWS)
def test_tiny_rows(n, monkeypatch):
    """one word, a word short by a bit, a full word, a second word of one bit"""
    check_case(tiny_case(n), monkeypatch)
