"""The evaluators and the data transforms above their launch caps.

Every kernel here launches a grid capped by `grid_for(items, block, max_blocks)` (csrc/common.h) and walks the rest
of its input in a grid-stride loop; the other GPU tests of these files stop below the cap, where every thread makes
one trip.  The sizes below start a second (and once a third) trip:

  eval_tally_kernel          > kTallyMaxGrid * kTallyBlock * 4 = 1 048 576 points (4 per thread, scalar tail)
  pan_insert_kernel          > 4096 * 256 = 1 048 576 points of one chunk (wave-uniform `i0 - lane` loop)
  eval_intersections_kernel  > 8192 * 256 = 2 097 152 mask points of one scan
  box_labels / box_runs      > 8192 * 256 = 2 097 152 points / mask points of one call
  train_data.hip             > blocks_for: 1024 * 256 = 262 144 points, quads (x4 split) or words / 4 (KITTI decode)

plus the scalar (`vec == false`) form of the quad loads behind unaligned pointers, and sg_train_id_set at exactly
kIdTable / 2 ids and one more.

The references are numpy on the host: np.bincount / np.unique / math.fsum written here in int64 / float64, or the
package's device='cpu' path (which the CPU suite pins to the reference's golden files).  Integers are compared
exactly.  Nothing is compared with a second run of the device path except where repeatability is the property.
tests/test_launch_caps.py reads the caps out of the sources and fails when a size below stops sitting on the side
of its cap it was chosen for.
"""
import collections
import contextlib
import io
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'golden'))

import pointwise_cases as pc  # noqa: E402
from softgroup_amd import _lib as L  # noqa: E402
from softgroup_amd import data  # noqa: E402
from softgroup_amd.data import TestTransform, TrainTransform  # noqa: E402
from softgroup_amd.data import _train_device as td  # noqa: E402
from softgroup_amd.data.test import _ROT  # noqa: E402
from softgroup_amd.data.train import blur_numpy, interp_numpy  # noqa: E402
from softgroup_amd.evaluation import (PanopticEval, ScanNetEval, evaluate_offset_mae, evaluate_semantic_acc,  # noqa: E402
                                      evaluate_semantic_miou)
from softgroup_amd.evaluation import det_eval as de  # noqa: E402
from softgroup_amd.evaluation import point_wise_eval as pw_mod  # noqa: E402
from softgroup_amd.evaluation.instance_eval import _runs_of  # noqa: E402
from softgroup_amd.util.rle import rle_encode_runs  # noqa: E402
from test_box_eval_gpu import _boxes_equal  # noqa: E402
from test_box_eval_gpu import _device_only as _boxes_device_only  # noqa: E402
from test_pointwise_eval_gpu import KITTI_STUFF, KITTI_THING, _pan_equal  # noqa: E402
from test_pointwise_eval_gpu import _device_only as _pan_device_only  # noqa: E402
from test_test_data import assert_item, blobs, kitti_yaml_map, labelled, voxel_cfg  # noqa: E402
from test_train_data import TOL  # noqa: E402
from test_train_data_gpu import SCANNET_CFG, _compare, _scannet  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# ----------------------------------------------------------------------------------------------------------------
# the sizes (tests/test_launch_caps.py checks them against the constants in the sources)
TALLY_CAP = 1048576                                  # kTallyMaxGrid * kTallyBlock * 4 points: the last one-trip size
TALLY_CASES = [(1048576, 'int64'), (1048577, 'int32'), (1049603, 'int64'), (2 * 1048576 + 4098, 'int32')]
PAN_CAP = 1048576                                    # pan_insert_kernel: 4096 * 256
PAN_SCANS, PAN_SCAN_POINTS = 9, 120000               # one chunk of 1 080 000 points
INTER_CAP = 2097152                                  # eval_intersections_kernel: 8192 * 256 mask points
INTER_POINTS, INTER_MASKS, INTER_MASK_POINTS = 600000, 40, 60000
INTER_ISOLATED = 20000                               # points of the mask of isolated points (one run each)
BOX_CAP = 2097152                                    # box_labels_kernel / box_runs_kernel: 8192 * 256
BOX_SCANS, BOX_SCAN_POINTS, BOX_MASKS = 8, 300000, 12
TRAIN_CAP = 262144                                   # blocks_for of train_data.hip: 1024 * 256 work items
TRAIN_SCANNET_N = 300000
TRAIN_S3DIS_N = 1100003                              # quarter subsample: 275 000 rows through gather_kernel
ELASTIC_N = 262144 + 257
X4_SIZES = [4 * 262144 + 1200, 4 * 262144 + 1200 + 3]
KITTI_CAP = 4 * 262144                               # kitti_decode_kernel: blocks_for over words / 4
KITTI_SIZES = [1048576, 1048576 + 1027]
UNALIGNED_N = 1003
ID_CAP = 8192                                        # _ID_CAP = kIdTable / 2
ID_LABELS = 20000
IGNORE = -100


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ----------------------------------------------------------------------------------------------------------------
# 1. the point-wise tally
def _tally_case(n, label_dtype):
    """one scan of n points: 20 classes, ~10 % of the gt and ~30 % of the instance labels ignored, predictions
    outside [0, MAX_CLASSES) among the rest -- the last 8 points carry one of everything, so that a tail that is
    dropped or counted twice changes a tally"""
    sp, sg, op, og, inst = pc.scannet_like(n % 1000 + 3, n)
    rng = np.random.default_rng(n)
    wild = rng.random(n) < 0.02
    sp[wild] = rng.choice([-1, -100, pw_mod.MAX_CLASSES, 70000, 2**31 - 1], int(wild.sum()))
    sg[-8:] = [3, 3, 19, IGNORE, 0, 7, 7, 5]
    sp[-8:] = [3, 4, 19, 3, -1, 7, pw_mod.MAX_CLASSES, 5]
    inst[-8:] = [1, IGNORE, 2, 3, IGNORE, 4, 5, 6]
    dt = np.dtype(label_dtype)
    return sp.astype(dt), sg.astype(dt), op, og, inst.astype(dt)


def _tally_reference(sp, sg, op, og, inst):
    """(seen, positive, correct) int64 [MAX_CLASSES], exact float64 offset sum, offset point count"""
    k = pw_mod.MAX_CLASSES
    sp, sg = sp.astype(np.int64), sg.astype(np.int64)
    valid = sg != IGNORE
    assert ((sg[valid] >= 0) & (sg[valid] < k)).all()
    seen = np.bincount(sg[valid], minlength=k)
    p = sp[valid]
    positive = np.bincount(p[(p >= 0) & (p < k)], minlength=k)
    correct = np.bincount(sg[valid][p == sg[valid]], minlength=k)
    pos = inst != IGNORE
    terms = np.abs(og[pos] - op[pos])                       # float32, as numpy and the kernel form them
    assert terms.dtype == np.float32
    return np.stack([seen, positive, correct]), math.fsum(terms.reshape(-1).astype(np.float64).tolist()), int(pos.sum())


@pytest.mark.parametrize('n,label_dtype', TALLY_CASES)
def test_class_tally_and_offset_sum_above_the_grid_cap(n, label_dtype):
    sp, sg, op, og, inst = _tally_case(n, label_dtype)
    assert pw_mod.chunks([n], pw_mod._CHUNK_POINTS) == [(0, 1)]              # one chunk, one launch
    assert 0.08 < (sg == IGNORE).mean() < 0.12 and ((sp < 0) | (sp >= pw_mod.MAX_CLASSES)).sum() > 1000
    tallies, off_sum, off_count = _tally_reference(sp, sg, op, og, inst)
    r = pw_mod._device_pass([sp], [sg], IGNORE, DEV)
    assert r is not None                                                     # no numpy fallback
    assert np.array_equal(r[0], tallies)
    runs = [pw_mod._device_pass(None, None, IGNORE, DEV, [inst], [op], [og]) for _ in range(2)]
    assert runs[0] is not None and runs[1] is not None
    assert int(runs[0][2]) == off_count
    # non-negative float64 terms: any summation order is within n_terms * 2**-53 of the exact sum, relatively
    n_terms = 3 * off_count
    err = abs(float(runs[0][1]) - off_sum)
    print(f'n={n} offset sum {float(runs[0][1])!r} exact {off_sum!r} rel err {err / off_sum:.3e} '
          f'bound {n_terms * 2.0**-53:.3e}')
    assert err <= n_terms * 2.0**-53 * off_sum
    assert np.float64(runs[0][1]).tobytes() == np.float64(runs[1][1]).tobytes()      # bitwise repeatable
    # both passes in one launch, and the evaluators on top of them
    both = pw_mod._device_pass([sp], [sg], IGNORE, DEV, [inst], [op], [og])
    assert both is not None and np.array_equal(both[0], tallies) and int(both[2]) == off_count
    assert np.float64(both[1]).tobytes() == np.float64(runs[0][1]).tobytes()
    assert evaluate_semantic_miou([sp], [sg], device=DEV) == evaluate_semantic_miou([sp], [sg], device='cpu')
    assert evaluate_semantic_acc([sp], [sg], device=DEV) == evaluate_semantic_acc([sp], [sg], device='cpu')
    mae = evaluate_offset_mae([op], [og], [inst], device=DEV)
    assert abs(mae - off_sum / off_count) <= n_terms * 2.0**-53 * (off_sum / off_count)
    mae_cpu = evaluate_offset_mae([op], [og], [inst], device='cpu')          # (numpy sums float32 pairwise)
    assert abs(mae - mae_cpu) <= 1e-5 * abs(mae_cpu)


# ----------------------------------------------------------------------------------------------------------------
# 2. PanopticEval: one chunk above the caps of pan_insert_kernel and of the tally's panoptic branch
def _table_of(ev, *args):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        res = ev.evaluate(*args)
    return res, out.getvalue()


@pytest.fixture(scope='module')
def panoptic_set():
    scans = [pc.kitti_like(300 + s, PAN_SCAN_POINTS) for s in range(PAN_SCANS)]
    preds, sems, insts = [list(x) for x in zip(*scans)]
    cpu, table = _table_of(PanopticEval(KITTI_THING, KITTI_STUFF, device='cpu'), preds, sems, insts)
    return preds, sems, insts, cpu, table


def test_panoptic_one_chunk_above_the_insert_cap(panoptic_set, monkeypatch):
    preds, sems, insts, cpu, table = panoptic_set
    ev = PanopticEval(KITTI_THING, KITTI_STUFF, device=DEV)
    sizes = [len(p) for p in preds]
    assert pw_mod.chunks(sizes, ev.max_chunk_points) == [(0, PAN_SCANS)] and sum(sizes) > PAN_CAP
    _pan_device_only(monkeypatch)
    gpu, gpu_table = _table_of(ev, preds, sems, insts)
    assert gpu_table == table and len(table.splitlines()) > len(KITTI_THING + KITTI_STUFF)
    _pan_equal(gpu, cpu)
    assert len(gpu) == len(cpu) == 10


# ----------------------------------------------------------------------------------------------------------------
# 3. instance-AP intersections (host backend of ScanNetEval): more mask points than one trip of the grid
CLASSES = tuple(f'class{i}' for i in range(1, 19))


def _intersection_scan():
    """600 000 points in 10 GT instances of 55 000 points (and unannotated stretches), 40 predictions of ~60 000
    points: one single long run, one of 20 000 isolated points, ten close to a GT instance (half of them with its
    class), the others a few runs each, some over points of no evaluated class"""
    n = INTER_POINTS
    rng = np.random.default_rng(17)
    gts = np.zeros(n, np.int64)
    for g in range(10):
        lo = 60000 * g
        gts[lo + 2000:lo + 57000] = (1 + g) * 1000 + g + 1
    gts[590000:] = 25000 + 77                              # a class that is not evaluated: void
    preds = []
    for p in range(INTER_MASKS):
        label = 1 + p % 18
        if p == 0:
            starts, lens = np.array([123457]), np.array([INTER_MASK_POINTS])
        elif p == 1:
            starts = 7 + 30 * np.arange(INTER_ISOLATED)
            lens = np.ones(INTER_ISOLATED, np.int64)
        elif p < 12:
            g = p - 2
            lo, hi = 60000 * g + int(rng.integers(0, 8000)), 60000 * (g + 1) - int(rng.integers(1, 8000))
            starts, lens = np.array([lo]), np.array([hi - lo])
            label = 1 + g if p % 2 else label
        else:
            k = int(rng.integers(3, 9))
            cuts = np.sort(rng.choice(np.arange(1, n // 100), 2 * k, replace=False)) * 100
            starts, lens = cuts[0::2], cuts[1::2] - cuts[0::2]
            lens = np.maximum(np.minimum(lens, lens * INTER_MASK_POINTS // int(lens.sum())), 1)     # ~60 000 in all
        preds.append(dict(scan_id='big', label_id=label, conf=np.float32(round(float(rng.random()), 2)),
                          pred_mask=rle_encode_runs(n, starts, lens)))
    return preds, gts


def _avgs_equal(a, b):
    if isinstance(b, dict):
        assert set(a) == set(b)
        for k in b:
            _avgs_equal(a[k], b[k])
    else:
        a, b = float(a), float(b)
        assert a == b or (math.isnan(a) and math.isnan(b)), (a, b)


def test_intersections_above_one_trip_of_mask_points():
    preds, gts = _intersection_scan()
    n = len(gts)
    runs = [_runs_of(p['pred_mask'], n) for p in preds]
    starts = np.concatenate([r[0] for r in runs])
    lens = np.concatenate([r[1] for r in runs])
    run_pred = np.concatenate([np.full(len(r[0]), k, np.int64) for k, r in enumerate(runs)])
    assert int(lens.sum()) > INTER_CAP and len(runs[0][0]) == 1 and (runs[1][1] == 1).all()
    assert (starts + lens <= n).all() and (starts >= 0).all()
    ids, inverse = np.unique(gts, return_inverse=True)
    n_slots = len(ids)
    gt_slot = inverse.reshape(-1).astype(np.int64)
    off = np.cumsum(lens) - lens
    points = np.arange(int(lens.sum())) + np.repeat(starts - off, lens)          # every mask point, in run order
    want = np.bincount(np.repeat(run_pred, lens) * n_slots + gt_slot[points],
                       minlength=len(preds) * n_slots).reshape(len(preds), n_slots)
    got = ScanNetEval(CLASSES, device=DEV)._count_matrix(starts, lens, run_pred, len(preds), gt_slot, n_slots)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert want.sum() == lens.sum() and (want[:, 0] > 0).any()
    a = ScanNetEval(CLASSES, device=DEV).evaluate([preds], [gts], verbose=False)
    b = ScanNetEval(CLASSES, device='cpu').evaluate([preds], [gts], verbose=False)
    _avgs_equal(a, b)
    assert b['all_ap_25%'] > 0 and b['all_rc_25%'] > 0


# ----------------------------------------------------------------------------------------------------------------
# 4. box extraction: every scan of a set in one call
def _box_scans(dtype, seed):
    """8 scans of 300 000 points in [-4, 4)^3, 40 GT instances each (runs and scattered points, ~10 % unlabelled),
    12 masks of three 25 000-point runs each per scan -> coords, masks as (starts, lens), labels"""
    rng = np.random.default_rng(seed)
    n = BOX_SCAN_POINTS
    coords, masks, insts = [], [], []
    for s in range(BOX_SCANS):
        coords.append(rng.uniform(-4, 4, (n, 3)).astype(dtype))
        inst = np.sort(rng.integers(0, 40, n))
        scatter = rng.random(n) < 0.3
        inst[scatter] = rng.integers(0, 40, int(scatter.sum()))
        inst[rng.random(n) < 0.1] = IGNORE
        inst[:40] = np.arange(40)[::-1]
        if s == BOX_SCANS - 1:
            inst[inst == 11] = IGNORE                   # an instance without points, in the second trip
        insts.append(inst.astype(np.int64))
        ms = []
        for _ in range(BOX_MASKS):
            m = np.zeros(n, bool)
            for lo in rng.integers(0, n - 25000, 3):
                m[lo:lo + 25000] = True
            m[rng.integers(0, n, 5)] = True             # a few single points
            ms.append(m)
        masks.append(ms)
    return coords, masks, insts


@pytest.mark.parametrize('dtype,rle', [(np.float32, True), (np.float64, False)])
def test_box_extraction_of_a_whole_set_in_one_call(dtype, rle, monkeypatch):
    coords, masks, insts = _box_scans(dtype, seed=3 + int(rle))
    sizes = [len(c) for c in coords]
    scan_off = np.concatenate([[0], np.cumsum(sizes)])
    mask_points = sum(int(m.sum()) for ms in masks for m in ms)
    assert scan_off[-1] > BOX_CAP and mask_points > BOX_CAP
    assert scan_off[BOX_SCANS - 1] >= BOX_CAP              # a scan boundary (and its owners' first points) in trip two
    assert min(float(c.min()) for c in coords) < -3.9
    if rle:
        masks = [[rle_encode_runs(len(m), *_runs_of(m, len(m))) for m in ms] for ms in masks]
    want = de.instance_boxes(coords, masks, insts, device='cpu')
    _boxes_device_only(monkeypatch)
    got = de.instance_boxes(coords, masks, insts, device=DEV)
    _boxes_equal(got, want)
    assert all(np.isfinite(p).all() and p.shape == (BOX_MASKS, 6) for p in got[0])
    for inst, (boxes, count, first) in zip(insts, got[1]):       # count and first against np.unique, exactly
        ids, idx, cnt = np.unique(inst[inst >= 0], return_index=True, return_counts=True)
        k = int(inst.max()) + 1
        exp_count, exp_first = np.zeros(k, np.int64), np.full(k, -1, np.int64)
        exp_count[ids], exp_first[ids] = cnt, np.flatnonzero(inst >= 0)[idx]
        assert np.array_equal(count, exp_count) and np.array_equal(first, exp_first)
        assert np.isnan(boxes[exp_count == 0]).all() and np.isfinite(boxes[exp_count > 0]).all()
    assert (got[1][-1][1] == 0).sum() == 1


# ----------------------------------------------------------------------------------------------------------------
# 5. the training transform
class _CountingLib:
    """the library with a call count per entry"""
    def __init__(self, lib):
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self.calls[name] += 1
            return fn(*a)
        return call


def _train_pair(cfg, raw, **kw):
    out = []
    for dev in ('cpu', DEV):
        np.random.seed(7)
        torch.manual_seed(7)
        out.append(TrainTransform(cfg, rng='numpy', device=dev, **kw)(*raw))
    return out


def test_train_transform_scannet_scan_above_the_block_cap(monkeypatch):
    lib = _CountingLib(L.lib())
    monkeypatch.setattr(L, 'lib', lambda: lib)
    raw = _scannet(n=TRAIN_SCANNET_N, seed=1)
    cpu, gpu = _train_pair(SCANNET_CFG, raw, dataset='scannetv2')
    _compare(cpu, gpu)
    kept = gpu[1].shape[0]
    print('scannet kept', kept, dict(lib.calls))
    assert SCANNET_CFG['min_npoint'] <= kept <= SCANNET_CFG['max_npoint'] < TRAIN_SCANNET_N      # a crop happened
    assert lib.calls['sg_train_elastic'] == 2 and lib.calls['sg_train_crop_count'] >= 1
    assert lib.calls['sg_train_compact'] == 1 and lib.calls['sg_train_gather'] == 0


def test_train_transform_s3dis_subsample_above_the_block_cap(monkeypatch):
    lib = _CountingLib(L.lib())
    monkeypatch.setattr(L, 'lib', lambda: lib)
    raw = _scannet(n=TRAIN_S3DIS_N, seed=2)
    assert int(TRAIN_S3DIS_N * 0.25) > TRAIN_CAP
    cpu, gpu = _train_pair(SCANNET_CFG, raw, dataset='s3dis', x4_split=True)
    _compare(cpu, gpu)
    kept = gpu[1].shape[0]
    print('s3dis kept', kept, dict(lib.calls))
    assert SCANNET_CFG['min_npoint'] <= kept < int(TRAIN_S3DIS_N * 0.25)                 # a crop happened
    assert lib.calls['sg_train_gather'] == 1 and lib.calls['sg_train_elastic'] == 2
    assert lib.calls['sg_train_crop_count'] >= 1 and lib.calls['sg_train_id_set'] == 2


def test_elastic_stage_through_the_c_abi_above_the_block_cap():
    """the recipe of test_blur_and_elastic_stages_through_the_c_abi at 262 144 + 257 points; both extrema of every
    axis lie behind point 262 144"""
    lib = L.lib()
    rng = np.random.default_rng(1)
    bb = (23, 17, 9)
    grids = np.stack([blur_numpy(g) for g in rng.standard_normal((3, ) + bb).astype(np.float32)])
    gran, mag = 6, 40.0
    half = np.array([(b - 1) * gran for b in bb], np.float64)
    n = ELASTIC_N
    x = rng.uniform(-1.05, 1.05, (n, 3)) * half            # (some points outside the grid: g = 0 there)
    x[:64] = np.round(x[:64] / 12) * 12                     # nodes
    x[TRAIN_CAP:TRAIN_CAP + 64] = np.round(x[TRAIN_CAP:TRAIN_CAP + 64] / 12) * 12
    x[-3], x[-5] = 1.5 * half, -1.4 * half                  # the extrema (outside the grid: they stay as they are)
    dx = torch.from_numpy(x.copy()).cuda()
    stats = torch.empty(9, dtype=torch.int64, device='cuda')
    L.check(lib.sg_train_elastic(L.ptr(dx), n, L.ptr(torch.from_numpy(grids).cuda()), *bb, float(gran), mag,
                                 L.ptr(stats), L.stream()), 'sg_train_elastic')
    got = dx.cpu().numpy()
    g = np.stack([interp_numpy(r, gran, x) for r in grids], 1)
    assert np.abs(g[TRAIN_CAP:]).max() > 0.01
    np.testing.assert_allclose((got - x) / mag, g, rtol=0, atol=1e-12)
    want = x + g * mag
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    h = td._decode(stats.cpu().numpy())
    assert np.array_equal(h[0:3], np.abs(got).max(0)) and np.array_equal(h[3:6], got.min(0))
    assert np.array_equal(h[6:9], got.max(0))
    assert np.array_equal(h[6:9], 1.5 * half) and np.array_equal(h[3:6], -1.4 * half)


# ----------------------------------------------------------------------------------------------------------------
# 6. the x4 split and the KITTI decode
@pytest.mark.parametrize('n', X4_SIZES)
def test_x4_split_above_the_block_cap_of_quads(n):
    xyz, rgb, inst = blobs(n, 40, 4 + n % 4, extent=(10.0, 8.0, 3.0))
    args = (xyz, rgb) + labelled(inst, 0, n_cls=13)
    vc = voxel_cfg('s3dis')
    got = TestTransform(vc, dataset='s3dis', x4_split=True)(*args, scan_id='x4')
    assert got[1].is_cuda and got[1].shape == (n, 4)
    assert_item(got, TestTransform(vc, dataset='s3dis', x4_split=True, device='cpu')(*args, scan_id='x4'), TOL, 'x4')


NO_KEY = int(data.KITTI_NO_KEY)


def _kitti_case(n, seed, missing_at=()):
    """n label words (class key | id << 16, negative words among them), the learning map's table, and the numpy
    decode; the words at `missing_at` carry key 99, which the map lacks"""
    lut = data.kitti_lut(kitti_yaml_map())
    keys = np.array(sorted(kitti_yaml_map()), np.int64)
    rng = np.random.default_rng(seed)
    words = ((rng.integers(0, 1 << 16, n) << 16) | keys[rng.integers(0, len(keys), n)]).astype(np.uint32)
    for i in missing_at:
        words[i] = (words[i] & np.uint32(0xFFFF0000)) | np.uint32(99)
    words = words.view(np.int32)
    assert lut[99] == NO_KEY and (words < 0).any()
    ent = lut[words & 0xFFFF].astype(np.int64)
    sem = np.where(ent == NO_KEY, -100, ent)
    inst = np.where((ent != NO_KEY) & (ent > 10), words.astype(np.int64), -100)
    return words, lut, sem, inst


@pytest.mark.parametrize('n', KITTI_SIZES)
def test_kitti_decode_above_the_block_cap(n):
    second = [i for i in (KITTI_CAP + 700, n - 3) if KITTI_CAP <= i < n]      # indices of the second trip
    for missing_at in ([], second, [700] + second, [n - 1]):
        words, lut, sem, inst = _kitti_case(n, n + len(missing_at), missing_at)
        missing = torch.full((1, ), 12345, dtype=torch.int64, device=DEV)
        d_sem, d_inst = td.decode_words(torch.device(DEV), words, t(lut), missing)
        assert np.array_equal(d_sem.cpu().numpy(), sem) and np.array_equal(d_inst.cpu().numpy(), inst)
        assert int(missing.item()) == (min(missing_at) if missing_at else -1), (n, missing_at)     # -1: all ones


# ----------------------------------------------------------------------------------------------------------------
# 7. unaligned inputs: the scalar form of the quad loads
def _shifted(a, dtype):
    """a copy of `a` one element into a larger device buffer: its pointer is NOT 16-byte aligned"""
    flat = np.ascontiguousarray(a, dtype).reshape(-1)
    buf = torch.zeros(flat.size + 8, dtype=torch.from_numpy(flat[:0]).dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + flat.size]
    view.copy_(torch.from_numpy(flat))
    assert view.data_ptr() % 16 != 0
    return view


def _x4_reference(xyz, scale):
    """xyz_middle (the fixed rotation, in the kernel's order of operations), the 12 minima of xyz_middle * scale per
    piece and axis, and the piece-major order of the points"""
    m = np.asarray(_ROT, np.float64)
    p = xyz.astype(np.float64)
    mid = (p[:, 0:1] * m[0] + p[:, 1:2] * m[1]) + p[:, 2:3] * m[2]
    mins = np.stack([(mid[b::4] * scale).min(0) for b in range(4)])
    order = np.concatenate([np.arange(b, len(xyz), 4) for b in range(4)])
    return mid, mins, order


def test_unaligned_inputs_take_the_scalar_loads():
    lib, n, scale = L.lib(), UNALIGNED_N, 50.0
    xyz, rgb, inst = blobs(n, 12, 8)
    sem, inst = (a.astype(np.int64) for a in labelled(inst, 0, n_cls=13))
    rot = _ROT
    mid, mins, order = _x4_reference(xyz, scale)
    # sg_test_x4_minima
    stats = []
    for x in (_shifted(xyz, np.float32), t(xyz)):
        block = torch.full((16, ), 5, dtype=torch.int64, device=DEV)
        L.check(lib.sg_test_x4_minima(L.ptr(x), n, rot.ctypes.data, scale, L.ptr(block), L.stream()), 'sg_test_x4_minima')
        stats.append(block.cpu().numpy())
    assert np.array_equal(stats[0], stats[1]) and stats[0][12] == 0 and (stats[0][13:] == 5).all()
    assert np.array_equal(td._decode(stats[0][:12]), mins.reshape(-1))
    # sg_test_x4_split (three features: the aligned call loads them as quads too)
    piece = np.repeat(np.arange(4), [len(range(b, n, 4)) for b in range(4)])
    w = mid[order] * scale - mins[piece]
    want = dict(coord=np.concatenate([piece[:, None], w.astype(np.int64)], 1), mid=mid[order], feat=rgb[order],
                sem=sem[order], inst=inst[order])
    outs = []
    for shift in (True, False):
        put = (lambda a, dt: _shifted(a, dt)) if shift else (lambda a, dt: t(np.ascontiguousarray(a, dt)))
        d_in = [put(xyz, np.float32), put(rgb, np.float32), put(sem, np.int64), put(inst, np.int64)]
        o = dict(coord=torch.full((n, 4), -7, dtype=torch.int64, device=DEV),
                 mid=torch.full((n, 3), -7, dtype=torch.float64, device=DEV),
                 feat=torch.full((n, 3), -7, dtype=torch.float32, device=DEV),
                 sem=torch.full((n, ), -7, dtype=torch.int64, device=DEV),
                 inst=torch.full((n, ), -7, dtype=torch.int64, device=DEV))
        L.check(lib.sg_test_x4_split(L.ptr(d_in[0]), L.ptr(d_in[1]), 3, L.ptr(d_in[2]), L.ptr(d_in[3]), n,
                                     rot.ctypes.data, scale, np.ascontiguousarray(mins).ctypes.data, L.ptr(o['coord']),
                                     L.ptr(o['mid']), L.ptr(o['feat']), L.ptr(o['sem']), L.ptr(o['inst']), L.stream()),
                'sg_test_x4_split')
        outs.append({k: v.cpu().numpy() for k, v in o.items()})
    for k in want:
        assert np.array_equal(outs[0][k], outs[1][k]), k
        assert np.array_equal(outs[0][k], want[k]) and outs[0][k].dtype == want[k].dtype, k
    # sg_kitti_decode_labels: unaligned words; aligned words with unaligned outputs
    words, lut, k_sem, k_inst = _kitti_case(n, 5, [n - 2])
    d_lut = t(lut)
    for shift_in, shift_out in ((True, False), (False, True), (False, False)):
        d_words = _shifted(words, np.int32) if shift_in else t(words)
        o_sem, o_inst = ((_shifted(np.full(n, -7), np.int64), _shifted(np.full(n, -7), np.int64)) if shift_out else
                         (torch.full((n, ), -7, dtype=torch.int64, device=DEV),
                          torch.full((n, ), -7, dtype=torch.int64, device=DEV)))
        missing = torch.full((1, ), 12345, dtype=torch.int64, device=DEV)
        L.check(lib.sg_kitti_decode_labels(L.ptr(d_words), n, L.ptr(d_lut), L.ptr(o_sem), L.ptr(o_inst), L.ptr(missing),
                                           L.stream()), 'sg_kitti_decode_labels')
        assert np.array_equal(o_sem.cpu().numpy(), k_sem) and np.array_equal(o_inst.cpu().numpy(), k_inst)
        assert int(missing.item()) == n - 2


# ----------------------------------------------------------------------------------------------------------------
# 8. the id set at its limit
def _labels_with_ids(k, seed):
    """20 000 int64 labels with exactly k distinct ids (gaps among them, the largest far above k) and some -100"""
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(3 * k, k, replace=False))
    ids[-1] = 10**12 + 7
    lab = ids[rng.integers(0, k, ID_LABELS)]
    lab[rng.choice(ID_LABELS, k, replace=False)] = ids                # every id present
    free = np.setdiff1d(np.arange(ID_LABELS), np.unique(lab, return_index=True)[1])
    lab[free[:500]] = IGNORE
    assert len(np.unique(lab[lab != IGNORE])) == k
    return lab.astype(np.int64)


@pytest.mark.parametrize('mode', ['fill_gaps', 'rank'])
def test_relabel_ids_with_exactly_the_id_cap(mode):
    lab = _labels_with_ids(ID_CAP, 1)
    d = t(lab)
    k, ids, mapped = td.relabel_ids(d, mode, torch.device(DEV))
    assert k == ID_CAP and np.array_equal(ids, np.unique(lab[lab != IGNORE]))
    want = data._fill_gaps(lab) if mode == 'fill_gaps' else data._rank_ids(lab)
    assert np.array_equal(d.cpu().numpy(), want)
    assert set(np.unique(want).tolist()) == set(range(ID_CAP)) | {IGNORE}


def test_one_id_more_than_the_cap_raises_and_writes_no_id_past_the_list():
    lab = _labels_with_ids(ID_CAP + 1, 2)
    d = t(lab)
    with pytest.raises(L.SoftGroupHipError):
        td.relabel_ids(d, 'fill_gaps', torch.device(DEV))
    assert np.array_equal(d.cpu().numpy(), lab)                       # labels untouched
    # the entry itself: the count says 8193, the list holds 8192 distinct ids of the set, nothing behind it
    lib = L.lib()
    meta = torch.full((1 + ID_CAP + 64, ), -7, dtype=torch.int64, device=DEV)
    ws = L.workspace(lib.sg_train_id_set_workspace_bytes(), DEV)
    L.check(lib.sg_train_id_set(L.ptr(d), len(lab), IGNORE, L.ptr(meta), ID_CAP, L.ptr(ws), ws.numel(), L.stream()),
            'sg_train_id_set')
    m = meta.cpu().numpy()
    assert m[0] == ID_CAP + 1 and (m[1 + ID_CAP:] == -7).all()
    listed = m[1:1 + ID_CAP]
    assert len(np.unique(listed)) == ID_CAP and np.isin(listed, lab[lab != IGNORE]).all()
