"""The fused losses, the mask IoU / label kernels and the instance extraction above their launch caps.

Every kernel here launches a capped grid and walks the rest of its input in a grid-stride loop (or, for
instance_npoint_kernel, in several 64-pair chunks per wave); the other GPU tests of these files stop below the
cap, where every thread makes one trip.  The sizes below start a second (and mostly a third) trip:

  pointwise_fwd_kernel       > T * kLossMaxBlocks rows, T = 256 for c <= 32, else 128: 262 144 / 131 072
  pointwise_bwd_kernel       > 4x that: 1 048 576 / 524 288 rows
  assign_rows / proposal_*   > 4 * 1024 = 4096 proposals (a wave per proposal); assign_cols: 4096 GT columns
  assign_labels / mask_fwd   > 262 144 proposals / mask points
  mask_bwd_kernel            > 8 * 262 144 = 2 097 152 elements of [m, k1]
  mask_iou / mask_label      > 8192 proposals (a workgroup per proposal), > kIouBins = 8192 instances (spill pass)
  instance_npoint_kernel     > 4096 waves x one 64-pair chunk = 262 144 pairs: several chunks per wave
  instance_bitmap / runs_emit / rle_text   > 4096 * 256 = 1 048 576 pairs / bitmap words / runs

The references are the ones of the files these kernels already have: the float64 torch formulas on the CPU
(test_fused_losses_gpu.py), the CPU oracle (mask IoU, bit-exact) and numpy written here (np.bincount, boolean
rows, rle_encode).  tests/test_launch_caps_train.py reads the caps out of the sources and fails when a size below
stops sitting on the side of its cap it was chosen for.  The optimizer's chunk walks are in
tests/test_fused_optim_gpu.py (_sizes_above).
"""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import oracle  # noqa: E402
from softgroup_amd import _lib as L  # noqa: E402
from softgroup_amd import ops  # noqa: E402
from softgroup_amd.util import rle_encode, rle_text_to_dicts  # noqa: E402
from test_fused_losses_gpu import IGN, LOSS_RTOL, _assign_check, _inst_case, _inst_check, _pw_case, _pw_check  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# ----------------------------------------------------------------------------------------------------------------
# the sizes (tests/test_launch_caps_train.py checks them against the constants in the sources)
PW_FWD_CAP = 262144                                  # pointwise_fwd_kernel, c <= 32: 256 rows * kLossMaxBlocks
PW_FWD_CAP_WIDE = 131072                             # ... c > 32: 128 rows * kLossMaxBlocks
PW_BWD_CAP = 4 * 262144                              # pointwise_bwd_kernel: 4 * kLossMaxBlocks workgroups
PW_BWD_CAP_WIDE = 4 * 131072
PW_CASES = [                                         # (n, c, weighted)
    (262144, 20, False),                             # the last one-trip size
    (262145, 20, False),                             # one row past the cap
    (2 * 262144 + 257, 13, True),                    # third trip, partial last tile
    (131072 + 129, 64, False),                       # the T = 128 form
    (524288 + 77, 33, True),                         # backward of the T = 128 form above its cap
    (1048576 + 321, 2, False),                       # backward of the T = 256 form above its cap
]
PW_TAIL_DEPTH = 30.0                                 # true-class logit of the last tile's rows: this far below the others
ROWS_CAP = 4096                                      # assign_rows / proposal_fwd / proposal_bwd: 4 waves * kLossMaxBlocks
COLS_CAP = 4096                                      # assign_cols_kernel, GT columns
LABELS_CAP = 262144                                  # assign_labels_kernel / mask_fwd_kernel: 256 * kLossMaxBlocks
ASSIGN_CASES = [                                     # (n_prop, n_gt)
    (4096, 130),                                     # the last one-trip size of the rows kernel
    (4097, 130),                                     # one proposal past that cap
    (8192 + 65, 7),                                  # third trip of the rows kernel
    (70, 4097),                                      # columns kernel above its cap
    (262145, 3),                                     # labels kernel above its cap
]
MASK_BWD_CAP = 8 * 262144                            # mask_bwd_kernel: elements of [m, k1]
INST_CASES = [                                       # (n_prop, k1, m)
    (4097, 19, 262144 + 257),                        # wave-per-proposal kernels and mask_fwd above cap; mask_bwd third trip
    (8200, 2, 1048576 + 70),                         # mask_bwd's second trip at k1 = 2
    (4096, 19, 262144),                              # the last one-trip sizes
]
IOU_PROP_CAP = 8192                                  # mask_iou_kernel / mask_label_kernel: min(nProposal, 8192) workgroups
IOU_BINS = 8192                                      # kIouBins: instances of one LDS histogram pass
IOU_MANY_PROPOSALS = dict(nP=8192 + 40, nI=37, N=60000)
IOU_MANY_INSTANCES = dict(nP=12, nI=8192 + 300, N=80000)
IOU_THRS = (0.0, 0.01, 0.5)
NPOINT_ONE_CHUNK_CAP = 262144                        # 4096 waves * 64 pairs
NPOINT_WAVES = 4096
NPOINT_MIN_PAIRS = 786432                            # above it every wave's range is >= 256 pairs = 4 chunks
NPOINT_GIANT = 150000
NPOINT_BLOCKS = dict(n64=2000, small=12000, mid=1700, dead=3000)
NPOINT_POINTS = 200000
NPOINT_CLASSES = [(5, 6), (19, 19)]                  # (nc, stride)
RUNS_CAP = 1048576                                   # instance_bitmap / instance_runs_emit / rle_text: 4096 * 256
RUNS_POINTS, RUNS_PROPOSALS, RUNS_PER_PROPOSAL = 40000, 1000, 1250
RUNS_MIN_NPOINT = 40
RUNS_THR = -0.46                                     # mask threshold of the runs case: 2 % of its class-0 scores below
RUNS_FULL_ROW, RUNS_DEAD, RUNS_DROPPED, RUNS_LONG = 3, 5, 7, (10, 500, 999)
MASK_THR = -0.5                                      # mask threshold of the npoint case


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ----------------------------------------------------------------------------------------------------------------
# 1. the point-wise loss
def _pw_tile(c):
    return 256 if c <= 32 else 128


def _pw_case_above(n, c, weighted):
    """_pw_case with the rows of the last tile made heavy.  A dropped or doubled tile of a few hundred rows in a
    million moves a mean by less than LOSS_RTOL; so every row of the last tile gets a valid label whose logit lies
    PW_TAIL_DEPTH = 30 below the row's smallest one (nll >= 30) -- and deeper where the tile has few rows (one, in
    three of the cases), so that the tile as a whole carries 2 % of n in nll.  -> case, rows of the last tile"""
    case = _pw_case(n, c, n % 1000 + c, weighted)
    tail = (n - 1) % _pw_tile(c) + 1
    depth = max(PW_TAIL_DEPTH, float(math.ceil(0.02 * n / tail)))
    y, s = case['y'][n - tail:], case['s'][n - tail:]                 # (views)
    y[y == IGN] = 0
    s[torch.arange(tail), y] = s.min(1).values - depth
    return case, tail


def _pw_loss_without_tail(case, tail):
    """the float64 semantic loss of all rows and of all rows but the last `tail`"""
    s, y = case['s'].double(), case['y']
    valid = y != IGN
    nll = -F.log_softmax(s[valid], 1).gather(1, y[valid][:, None]).squeeze(1)
    w = torch.ones_like(nll) if case['w'] is None else case['w'].double()[y[valid]]
    k = int(valid[:len(y) - tail].sum())
    assert int(valid[len(y) - tail:].sum()) == tail
    return float((w * nll).sum() / w.sum()), float((w[:k] * nll[:k]).sum() / w[:k].sum()), float(nll[k:].min())


@pytest.mark.parametrize('n,c,weighted', PW_CASES)
def test_point_wise_loss_above_the_grid_caps(n, c, weighted):
    case, tail = _pw_case_above(n, c, weighted)
    full, cut, tail_nll = _pw_loss_without_tail(case, tail)
    print(f'n={n} c={c} tail {tail} rows, nll >= {tail_nll:.1f}: loss {full!r}, without the tail {cut!r}, '
          f'relative {abs(full - cut) / abs(full):.3e}')
    assert tail_nll >= PW_TAIL_DEPTH
    assert abs(full - cut) > 3 * LOSS_RTOL * abs(full)                # (a case that fails here has the wrong inputs)
    out, d_s, d_o = _pw_check(case, f'n={n} c={c} w={weighted}')
    assert abs(float(out[4]) - full) <= LOSS_RTOL * abs(full)
    if not weighted:                                                  # sum w is a count: exact
        assert float(out[1]) == float((case['y'] != IGN).sum())
    assert float(out[3]) == float((case['inst'] != IGN).sum())


# ----------------------------------------------------------------------------------------------------------------
# 2. the assignment
def _assign_case(n_prop, n_gt):
    """the IoUs of test_assignment_shapes: eighths (many exact ties), 35 % zeros, first column equal to the last"""
    g = torch.Generator().manual_seed(n_prop * 1000 + n_gt)
    ious = (torch.rand(n_prop, n_gt, generator=g) * 8).round() / 8
    ious[torch.rand(n_prop, n_gt, generator=g) < 0.35] = 0
    if n_gt > 1:
        ious[:, 0] = ious[:, -1]
    cls = torch.randint(0, 18, (n_gt, ), generator=g)
    cls[torch.rand(n_gt, generator=g) < 0.3] = IGN
    cls[n_gt // 2] = 3
    return ious, cls


@pytest.mark.parametrize('n_prop,n_gt', ASSIGN_CASES)
def test_assignment_above_the_grid_caps(n_prop, n_gt):
    ious, cls = _assign_case(n_prop, n_gt)
    _assign_check(ious, cls, (n_prop, n_gt))


# ----------------------------------------------------------------------------------------------------------------
# 3. proposal and mask losses
@pytest.mark.parametrize('n_prop,k1,m', INST_CASES)
def test_proposal_and_mask_losses_above_the_grid_caps(n_prop, k1, m):
    _inst_check(_inst_case(n_prop, k1, m, 7 * n_prop + k1 + m % 1000), f'P={n_prop} K+1={k1} M={m}')


# ----------------------------------------------------------------------------------------------------------------
# 4. mask IoU and mask label
def _iou_many_proposals():
    """8232 proposals of 0 .. 40 points on 37 instances.  Workgroup b takes proposals b and b + 8192 and reuses its
    LDS histogram and point total: for b < 40 proposal b is 40 points of ONE instance, proposal b + 8192 is empty
    (even b) or three points of another instance (odd b) -- a histogram that is not cleared shows at once"""
    nP, nI, N = (IOU_MANY_PROPOSALS[k] for k in ('nP', 'nI', 'N'))
    rng = np.random.default_rng(29)
    inst = rng.integers(0, nI, N).astype(np.int64)
    inst[rng.random(N) < 0.03] = -100
    lens = rng.integers(0, 41, nP)
    lens[::97] = 0
    second = nP - IOU_PROP_CAP
    lens[:second] = 40
    lens[IOU_PROP_CAP:] = np.where(np.arange(second) % 2 == 0, 0, 3)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    pidx = rng.integers(0, N, off[-1]).astype(np.int32)
    for b in range(second):
        pidx[off[b]:off[b + 1]] = rng.choice(np.flatnonzero(inst == b % nI), 40, replace=False)
        p = IOU_PROP_CAP + b
        pidx[off[p]:off[p + 1]] = rng.choice(np.flatnonzero(inst == (b + 5) % nI), lens[p], replace=False)
    cls = rng.integers(0, 18, nI).astype(np.int64)
    cls[[3, 9]] = -100
    return inst, off, pidx, cls


def _iou_many_instances():
    """12 proposals of 500 .. 3000 points on 8492 instances: labels on both sides of bin 8192.  Instances 8191,
    8192, 8300 and 5 are blocks of several hundred points with a proposal around each; instance 8400 (more points
    inside its proposal than instance 100, but class -100) must lose the arg-max"""
    nP, nI, N = (IOU_MANY_INSTANCES[k] for k in ('nP', 'nI', 'N'))
    rng = np.random.default_rng(31)
    inst = rng.integers(0, nI, N).astype(np.int64)
    inst[rng.random(N) < 0.03] = -100
    blocks = {IOU_BINS - 1: (0, 600), IOU_BINS: (600, 1200), 8300: (1200, 2000), 5: (2000, 2700), 8400: (2700, 3300),
              100: (3300, 3700)}
    for g, (lo, hi) in blocks.items():
        inst[inst == g] = -100
        inst[lo:hi] = g
    props = []
    for p in range(nP):
        noise = rng.integers(3700, N, int(rng.integers(500, 3001)))
        if p < 4:
            lo, hi = blocks[[IOU_BINS - 1, IOU_BINS, 8300, 5][p]]
            props.append(np.concatenate([np.arange(lo, hi), noise[:400]]))
        elif p == 4:                                    # half of 8191, two thirds of 8192
            props.append(np.concatenate([np.arange(0, 300), np.arange(600, 1000), noise[:300]]))
        elif p == 5:
            props.append(np.concatenate([np.arange(2700, 3300), np.arange(3300, 3700), noise[:500]]))
        else:
            props.append(noise)
    lens = np.array([len(q) for q in props])
    assert lens.min() >= 500 and lens.max() <= 3000
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    pidx = np.concatenate([rng.permutation(q) for q in props]).astype(np.int32)
    cls = rng.integers(0, 18, nI).astype(np.int64)
    cls[rng.random(nI) < 0.1] = -100
    cls[[IOU_BINS - 1, IOU_BINS, 8300, 5, 100]] = [1, 2, 3, 4, 5]
    cls[[8400, 7, IOU_BINS + 7]] = -100
    return inst, off, pidx, cls


def _iou_check(inst, off, pidx, cls, nI):
    pointnum = np.bincount(inst[inst >= 0], minlength=nI).astype(np.int32)
    sig = np.random.default_rng(len(pidx)).random(len(pidx)).astype(np.float32)
    ref = oracle.get_mask_iou_on_cluster(pidx, off, inst, pointnum)
    iou = ops.get_mask_iou_on_cluster(t(pidx), t(off), t(inst), t(pointnum))
    assert np.array_equal(iou.cpu().numpy(), ref)
    ref2 = oracle.get_mask_iou_on_pred(pidx, off, inst, pointnum, sig)
    iou2 = ops.get_mask_iou_on_pred(t(pidx), t(off), t(inst), t(pointnum), t(sig))
    assert np.array_equal(iou2.cpu().numpy(), ref2)
    assert not np.array_equal(ref, ref2)
    labels = []
    for thr in IOU_THRS:
        want = oracle.get_mask_label(pidx, off, inst, cls, pointnum, ref, thr)
        ml = ops.get_mask_label(t(pidx), t(off), t(inst), t(cls), t(pointnum), iou, thr)
        assert np.array_equal(ml.cpu().numpy(), want), thr
        labels.append(want)
    return ref, labels


def test_mask_iou_and_label_with_more_proposals_than_workgroups():
    inst, off, pidx, cls = _iou_many_proposals()
    nP, nI = IOU_MANY_PROPOSALS['nP'], IOU_MANY_PROPOSALS['nI']
    lens = np.diff(off)
    assert len(lens) == nP > IOU_PROP_CAP and lens.max() == 40 and (lens == 0).sum() > 20
    assert 0.02 < (inst == -100).mean() < 0.04
    ref, labels = _iou_check(inst, off, pidx, cls, nI)
    second = nP - IOU_PROP_CAP
    differ = sum(int(np.argmax(ref[b]) != np.argmax(ref[IOU_PROP_CAP + b]) or ref[IOU_PROP_CAP + b].max() == 0)
                 for b in range(second))
    assert differ == second and (ref[:second].max(1) > 0.01).all()
    # the three thresholds label differently: 0.0 labels every proposal's points, 0.5 next to none
    assert (labels[0] >= 0).all() and (labels[1] == 1).sum() > (labels[2] == 1).sum() and (labels[2] == -1).any()


def test_mask_iou_and_label_with_more_instances_than_histogram_bins():
    inst, off, pidx, cls = _iou_many_instances()
    nP, nI = IOU_MANY_INSTANCES['nP'], IOU_MANY_INSTANCES['nI']
    assert nI > IOU_BINS and (inst[pidx] >= IOU_BINS).sum() > 1000 and (inst[pidx] < IOU_BINS).sum() > 1000
    assert (inst[pidx] == IOU_BINS - 1).sum() >= 600 and (inst[pidx] == IOU_BINS).sum() >= 600
    assert (cls[:IOU_BINS] == -100).sum() > 100 and (cls[IOU_BINS:] == -100).sum() > 10
    ref, labels = _iou_check(inst, off, pidx, cls, nI)
    arg = np.argmax(np.where(cls[None, :] != -100, ref, -1.0), 1)                # the oracle's arg-max column
    print('arg-max instance per proposal', arg.tolist())
    assert arg[0] == IOU_BINS - 1 and arg[1] == IOU_BINS and arg[2] == 8300 and arg[3] == 5
    assert (arg >= IOU_BINS).any()                                              # a best IoU in the spill pass
    assert np.argmax(ref[5]) == 8400 and arg[5] == 100                          # the ignored instance loses
    assert (labels[2] == 1).sum() >= 600 + 600 + 800 + 700


# ----------------------------------------------------------------------------------------------------------------
# 5. instance extraction: sg_instance_npoint with several chunks per wave
def _npoint_layout():
    """proposal sizes, in order: one giant; (a filler up to a multiple of 64;) proposals of exactly 64 pairs -- a
    proposal change at every chunk boundary; sizes 1 .. 30 -- mixed chunks; sizes 100 .. 400 -- uniform and mixed
    chunks alternate; one proposal without a score above the threshold; a last one that ends 7 pairs into a chunk.
    -> sizes, index of the proposal without scores"""
    rng = np.random.default_rng(7)
    sizes = [NPOINT_GIANT]
    if NPOINT_GIANT % 64:
        sizes.append(-NPOINT_GIANT % 64)
    sizes += [64] * NPOINT_BLOCKS['n64']
    sizes += rng.integers(1, 31, NPOINT_BLOCKS['small']).tolist()
    sizes += rng.integers(100, 401, NPOINT_BLOCKS['mid']).tolist()
    dead = len(sizes)
    sizes.append(NPOINT_BLOCKS['dead'])
    sizes.append((7 - sum(sizes)) % 64 + 192)
    return np.asarray(sizes, np.int64), dead


def npoint_wave_range(S):
    """pairs per wave of instance_npoint_kernel: ceil(S / 4096) rounded up to whole chunks"""
    return (-(-S // NPOINT_WAVES) + 63) // 64 * 64


@pytest.fixture(scope='module')
def npoint_pairs():
    sizes, dead = _npoint_layout()
    prop = np.repeat(np.arange(len(sizes)), sizes)
    rng = np.random.default_rng(8)
    pairs = np.stack([prop, rng.integers(0, NPOINT_POINTS, len(prop))], 1).astype(np.int32)
    pairs.setflags(write=False)
    return sizes, dead, pairs


def test_npoint_layout_reaches_every_transition_of_the_chunk_walk(npoint_pairs):
    """from the layout alone: what the waves of the kernel meet on their way through their ranges"""
    sizes, dead, pairs = npoint_pairs
    S = len(pairs)
    per = npoint_wave_range(S)
    assert S > NPOINT_MIN_PAIRS > NPOINT_ONE_CHUNK_CAP and per >= 256 and S % 64 == 7
    assert (NPOINT_WAVES - 1) * per >= S                                        # trailing waves start past S
    first = pairs[0::64, 0]                                                     # chunks are 64-aligned: per % 64 == 0
    last = pairs[np.minimum(np.arange(63, S + 63, 64), S - 1), 0]
    uniform = first == last                                                     # (pairs are grouped by proposal)
    same_wave = (np.arange(1, len(first)) % (per // 64)) != 0                   # chunk i - 1 and chunk i in one range
    a, b = slice(0, -1), slice(1, None)
    assert (same_wave & uniform[a] & uniform[b] & (first[a] == first[b])).any()     # carry across chunks
    assert (same_wave & uniform[a] & uniform[b] & (first[a] != first[b])).any()     # flush on a change at a boundary
    assert (same_wave & ~uniform[a] & uniform[b]).any()                             # uniform after the fall-back
    assert (same_wave & uniform[a] & ~uniform[b]).any()                             # flush before the fall-back
    head = 1 + (NPOINT_GIANT % 64 != 0)                                         # the giant and its filler
    assert sizes[:head].sum() % 64 == 0 and (sizes[head:head + NPOINT_BLOCKS['n64']] == 64).all()


@pytest.mark.parametrize('nc,stride', NPOINT_CLASSES)
def test_instance_npoint_with_several_chunks_per_wave(npoint_pairs, nc, stride):
    lib = L.lib()
    sizes, dead, pairs = npoint_pairs
    S, nP = len(pairs), len(sizes)
    ms = np.random.default_rng(nc).standard_normal((S, stride), dtype=np.float32)
    ms[pairs[:, 0] == dead] = -9.0
    want = np.stack([np.bincount(pairs[ms[:, i] > MASK_THR, 0], minlength=nP) for i in range(nc)], 1)
    assert want[0].min() > 90000 and (want[dead] == 0).all() and want.sum() > nc * S // 2
    d_pairs, d_ms = t(pairs), t(ms)
    runs = []
    for _ in range(2):
        npoint = torch.full((nP, nc), -7, dtype=torch.int32, device=DEV)
        L.check(lib.sg_instance_npoint(L.ptr(d_pairs), L.ptr(d_ms), S, stride, nc, MASK_THR, nP, L.ptr(npoint),
                                       L.stream()), 'sg_instance_npoint')
        runs.append(npoint.cpu().numpy())
    assert np.array_equal(runs[0], want)
    assert np.array_equal(runs[1], want)


# ----------------------------------------------------------------------------------------------------------------
# 6. instance extraction: bitmap, runs and RLE text above 1 048 576 pairs / words / runs
def _runs_case():
    """1000 proposals of 1250 distinct random points of 40 000 (nearly every point its own run); proposal 3 holds
    every point, proposal 5 has no score above the threshold, proposals 10, 500 and 999 a run of 300 points that
    starts inside a 32-bit word.  -> pairs [S, 2], mask_scores [S, 2]"""
    rng = np.random.default_rng(43)
    N = RUNS_POINTS
    pairs = []
    for p in range(RUNS_PROPOSALS):
        if p == RUNS_FULL_ROW:
            q = rng.permutation(N)
        elif p in RUNS_LONG:
            a = int(rng.integers(0, N - 400)) // 32 * 32 + 20
            q = rng.permutation(np.union1d(np.arange(a, a + 300), rng.choice(N, RUNS_PER_PROPOSAL - 300, replace=False)))
        else:
            q = rng.choice(N, RUNS_PER_PROPOSAL, replace=False)                 # (BFS order is not sorted)
        pairs.append(np.stack([np.full(len(q), p), q], 1))
    pairs = np.concatenate(pairs).astype(np.int32)
    ms = rng.random((len(pairs), 2), dtype=np.float32) - 0.48                   # uniform in [-0.48, 0.52): 2 % below RUNS_THR
    ms[pairs[:, 0] == RUNS_DEAD] = -9.0
    for p in RUNS_LONG + (RUNS_FULL_ROW, ):
        ms[pairs[:, 0] == p, 0] = 1.0
    return pairs, ms


def test_instance_runs_and_rle_text_above_one_trip():
    lib = L.lib()
    N, nP, nc = RUNS_POINTS, RUNS_PROPOSALS, 2
    words = (N + 31) // 32
    pairs, ms = _runs_case()
    S = len(pairs)
    on = ms[:, 0] > RUNS_THR
    count = np.stack([np.bincount(pairs[ms[:, i] > RUNS_THR, 0], minlength=nP) for i in range(nc)])      # [nc, nP]
    keep = np.zeros((nc, nP), bool)
    keep[0] = count[0] >= RUNS_MIN_NPOINT                  # every (class 0, proposal) with enough points
    keep[0, RUNS_DROPPED] = False
    assert not keep[0, RUNS_DEAD] and count[0, RUNS_DEAD] == 0 and count[0, RUNS_FULL_ROW] == N
    kept = np.argwhere(keep)                               # class-major
    n_kept = len(kept)
    assert n_kept == nP - 2 and S > RUNS_CAP and n_kept * words > RUNS_CAP
    inst_of = np.full((nc, nP), -1, np.int32)
    inst_of[kept[:, 0], kept[:, 1]] = np.arange(n_kept)
    # the reference: one boolean row per kept instance, its 0 -> 1 and 1 -> 0 edges
    dense = np.zeros((nP, N), bool)
    dense[pairs[on, 0], pairs[on, 1]] = True
    rows = dense[kept[:, 1]]
    pad = np.zeros((n_kept, N + 2), np.int8)
    pad[:, 1:-1] = rows
    edge = np.diff(pad, axis=1)
    r_s, want_st = np.nonzero(edge == 1)
    _, want_en = np.nonzero(edge == -1)
    want_b = np.concatenate([[0], np.cumsum(np.bincount(r_s, minlength=n_kept))])
    n_runs = len(want_st)
    assert n_runs > RUNS_CAP and len(want_en) == n_runs                          # from the reference alone
    k_full = int(inst_of[0, RUNS_FULL_ROW])
    assert want_b[k_full + 1] - want_b[k_full] == 1 and want_en[want_b[k_full]] == N
    for p in RUNS_LONG:
        k = int(inst_of[0, p])
        lens = (want_en - want_st)[want_b[k]:want_b[k + 1]]
        assert lens.max() >= 300 and want_st[want_b[k]:want_b[k + 1]][np.argmax(lens)] % 32 != 0
    # the device
    d_pairs, d_ms, d_inst = t(pairs), t(ms), t(inst_of)
    npoint = torch.full((nP, nc), -7, dtype=torch.int32, device=DEV)
    L.check(lib.sg_instance_npoint(L.ptr(d_pairs), L.ptr(d_ms), S, 2, nc, RUNS_THR, nP, L.ptr(npoint), L.stream()),
            'sg_instance_npoint')
    assert np.array_equal(npoint.cpu().numpy(), count.T)
    cap = int(count[keep].sum())
    assert cap >= n_runs
    starts = torch.full((cap, ), -7, dtype=torch.int32, device=DEV)
    ends = torch.full((cap, ), -7, dtype=torch.int32, device=DEV)
    bounds = torch.full((n_kept + 1, ), -7, dtype=torch.int64, device=DEV)
    ws = L.workspace(lib.sg_instance_runs_workspace_bytes(n_kept, N), DEV)
    L.check(lib.sg_instance_runs(L.ptr(d_pairs), L.ptr(d_ms), S, 2, nc, RUNS_THR, L.ptr(d_inst), nP, n_kept, N,
                                 L.ptr(starts), L.ptr(ends), L.ptr(bounds), cap, L.ptr(ws), ws.numel(), L.stream()),
            'sg_instance_runs')
    assert np.array_equal(bounds.cpu().numpy(), want_b)
    st, en = starts.cpu().numpy(), ends.cpu().numpy()
    assert np.array_equal(st[:n_runs], want_st) and np.array_equal(en[:n_runs], want_en)
    assert (st[n_runs:] == -7).all() and (en[n_runs:] == -7).all()              # nothing behind the last run
    # the text of the same runs, written on the device, equals rle_encode of the dense rows
    tcap = int(lib.sg_rle_format_device_text_bytes(cap, N))
    text = torch.empty(tcap, dtype=torch.uint8, device=DEV)
    text_off = torch.empty(n_kept + 1, dtype=torch.int64, device=DEV)
    ws2 = L.workspace(lib.sg_rle_format_device_workspace_bytes(cap), DEV)
    L.check(lib.sg_rle_format_device(L.ptr(starts), L.ptr(ends), L.ptr(bounds), n_kept, cap, N, L.ptr(text), tcap,
                                     L.ptr(text_off), L.ptr(ws2), ws2.numel(), L.stream()), 'sg_rle_format_device')
    got = rle_text_to_dicts(N, text, text_off.cpu().tolist())
    assert len(got) == n_kept
    for k in range(n_kept):
        assert got[k] == rle_encode(rows[k]), k
