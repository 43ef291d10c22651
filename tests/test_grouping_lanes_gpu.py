"""Lane-group widths of the grouping head's list kernels (sg_grouping_set_lanes): the ball query and the
clustering must equal the CPU oracle bit for bit -- neighbour lists, both columns of start_len, cluster
membership and member order -- for every forced width (8, 16, 32, 64 lanes per node) and for the automatic
choice.

Inputs (r = 0.04 throughout):
  sparse   4000 points uniform in a 0.75 m cube: lists of 1..11 entries, mean 3.4 (scattered points);
  mixed    six Gaussian blobs plus 3000 uniform points: 3794 points, lists of 1..117 entries with every
           length around 8, 16, 32 and 64 present and 174 lists above 64 (the fill pass's work list);
  capped   1500 points inside a few millimetres: every list at the 1000 cap, so every edge takes the
           symmetric-edge check inside narrow groups (widths 8 and 64);
  halves   the sparse cloud shifted to negative coordinates, two batch segments;
  tiny     1, 5, 9, 63 and 65 points: fewer nodes than one wave holds, no multiple of 64 / lanes."""
import functools

import numpy as np
import pytest
import torch

import oracle
from softgroup_amd import _lib as L
from softgroup_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda'
R = 0.04
WIDTHS = (8, 16, 32, 64, 0)          # 0 = automatic
MEAN = np.array([-1.0], np.float32)   # class 0 without a mean: the threshold is a point count

_BLOBS = ((0.03, 300), (0.02, 120), (0.05, 200), (0.015, 70), (0.04, 64), (0.03, 40))


def _sparse_and_mixed():
    rng = np.random.default_rng(11)
    sparse = (rng.random((4000, 3)) * 0.75).astype(np.float32)
    ctr = rng.random((len(_BLOBS), 3)) * 0.75
    pts = [ctr[i] + rng.normal(0, s, (m, 3)) for i, (s, m) in enumerate(_BLOBS)]
    pts.append(rng.random((3000, 3)) * 1.5)
    mixed = np.concatenate(pts).astype(np.float32)
    return sparse, mixed[rng.permutation(len(mixed))]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(xyz, batch_idxs, batch_offsets, threshold) and the oracle's results, computed once per input."""
    if name in ('sparse', 'mixed', 'halves'):
        sparse, mixed = _sparse_and_mixed()
        xyz = mixed if name == 'mixed' else sparse
        if name == 'halves':
            xyz = xyz - np.float32(0.4)
        thr = 5.0
    elif name == 'capped':
        xyz = np.random.default_rng(11).normal(0, 0.002, (1500, 3)).astype(np.float32)
        thr = 2.0
    else:                                   # tiny<n>: dense enough that the few points do have neighbours
        n = int(name[4:])
        xyz = (np.random.default_rng(n).random((n, 3)) * 0.1).astype(np.float32)
        thr = 1.0
    n = len(xyz)
    bi = np.zeros(n, np.int32)
    if name == 'halves':
        bi[n // 2:] = 1
    bo = np.concatenate([[0], np.cumsum(np.bincount(bi))]).astype(np.int32)
    ridx, rsl = oracle.ballquery_batch_p(xyz, bi, bo, R, 300)
    rci, rco = oracle.bfs_cluster(MEAN, ridx, rsl, thr, 0)
    for a in (xyz, bi, bo, ridx, rsl, rci, rco):
        a.setflags(write=False)
    return xyz, bi, bo, thr, ridx, rsl, rci, rco


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)           # (a copy: the cached inputs are read-only)


def _check(name, lanes):
    xyz, bi, bo, thr, ridx, rsl, rci, rco = _case(name)
    lib = L.lib()
    prev = lib.sg_grouping_set_lanes(lanes)
    assert prev >= 0
    try:
        idx, sl = ops.ballquery_batch_p(_t(xyz), _t(bi), _t(bo), R, 300)
        assert np.array_equal(sl.cpu().numpy()[:, 1], rsl[:, 1])
        assert np.array_equal(sl.cpu().numpy()[:, 0], rsl[:, 0])
        assert np.array_equal(idx.cpu().numpy(), ridx)
        ci, co = ops.bfs_cluster(torch.from_numpy(MEAN), idx, sl, thr, 0)
        assert np.array_equal(co.cpu().numpy(), rco)
        assert np.array_equal(ci.cpu().numpy(), rci)         # membership AND member order
    finally:
        lib.sg_grouping_set_lanes(prev)
    return rsl, rco


@pytest.mark.parametrize('lanes', WIDTHS)
def test_sparse_lists(lanes):
    rsl, rco = _check('sparse', lanes)
    assert rsl[:, 1].min() == 1 and rsl[:, 1].max() == 11 and abs(rsl[:, 1].mean() - 3.4) < 0.05


@pytest.mark.parametrize('lanes', WIDTHS)
def test_mixed_lists_cover_every_boundary(lanes):
    rsl, rco = _check('mixed', lanes)
    ln = rsl[:, 1]
    assert len(ln) == 3794 and ln.min() == 1 and ln.max() == 117
    for k in (7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65):
        assert (ln == k).any(), k
    assert (ln > 64).sum() == 174                    # these take the work-list path of the fill
    assert len(rco) - 1 == 6 and rco[-1] == 780


@pytest.mark.parametrize('lanes', (8, 64))
def test_capped_lists_symmetric_edge_check(lanes):
    rsl, rco = _check('capped', lanes)
    assert (rsl[:, 1] == 1000).all()


@pytest.mark.parametrize('lanes', WIDTHS)
def test_two_segments_negative_coordinates(lanes):
    _check('halves', lanes)


@pytest.mark.parametrize('n', (1, 5, 9, 63, 65))
@pytest.mark.parametrize('lanes', WIDTHS)
def test_tiny_n(lanes, n):
    _check('tiny%d' % n, lanes)


def test_setter_returns_the_previous_value_and_rejects_other_widths():
    lib = L.lib()
    prev = lib.sg_grouping_set_lanes(16)
    try:
        assert lib.sg_grouping_set_lanes(8) == 16
        assert lib.sg_grouping_set_lanes(12) < 0          # refused, nothing changed
        assert lib.sg_grouping_set_lanes(0) == 8
    finally:
        lib.sg_grouping_set_lanes(prev)
