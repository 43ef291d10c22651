"""Oriented box IoU, box NMS and oriented box AP, numpy side (softgroup_amd.ops.boxes, util.boxes, evaluation.det_eval):
the scalar definition against exact arithmetic, against ``get_iou`` on axis-aligned boxes and against its invariants;
the vectorised twin against the scalar definition byte for byte; the NMS twin and the matching against plain loops;
oriented AP against axis-aligned AP; and the sizes of tests/test_box_ops_gpu.py against the caps in box_ops.hip.

Bounds.  Areas are held to exact arithmetic within 1e-12 of the larger rectangle: three orders above the rounding
error of the definition (a few 1e-16, written to profiles/box_ops_parity.txt), three below the first error of a wrong
formula.  IoUs of equal or mirrored configurations are held within 1e-12 for the same reason."""
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import box_cases as C  # noqa: E402
import test_box_ops_gpu as G  # noqa: E402

from softgroup_amd.evaluation import det_eval as de  # noqa: E402
from softgroup_amd.evaluation import (eval_det_cls, evaluate_box_ap, get_iou, get_iou_bev,  # noqa: E402
                                      get_iou_obb)
from softgroup_amd.ops import boxes as BX  # noqa: E402
from softgroup_amd.util import ObjectTable, nms_boxes, nms_objects, take_rows  # noqa: E402

ROOT = os.path.dirname(HERE)
MODES = ('3d', 'bev')


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


# ---- 1. exact reference ---------------------------------------------------------------------------------------------------
def test_area_against_exact_arithmetic():
    pairs = C.exact_pairs(11, 5000)
    worst, overlap = 0.0, 0
    for a, b in pairs:
        fa, fb = C.to_float(a), C.to_float(b)
        got = BX._area_pair(fa, fb)
        want = C.exact_area(a, b)
        scale = max(fa[3] * fa[4], fb[3] * fb[4])
        err = abs(Fraction(got) - want) / Fraction(scale)
        worst = max(worst, float(err))
        overlap += want > 0
    print(f'worst |area - exact| / max area = {worst:.3e}; {overlap} of {len(pairs)} pairs overlap')
    try:
        with open(os.path.join(ROOT, 'profiles', 'box_ops_parity.txt'), 'w') as f:
            f.write('# tests/test_box_ops.py::test_area_against_exact_arithmetic: the float64 rectangle clip of\n'
                    '# softgroup_amd.ops.boxes against the same clip in fractions.Fraction, rotations from Pythagorean\n'
                    '# triples, centres and extents multiples of 1/64; bound 1e-12\n'
                    f'pairs {len(pairs)}   overlapping {overlap}\n'
                    f'worst |area_float - area_exact| / max(du_a dv_a, du_b dv_b) = {worst:.3e}\n')
    except OSError:
        pass
    assert 3 * overlap >= len(pairs), overlap                 # the test must not pass on zeros
    assert worst <= 1e-12, worst


# ---- 2. against get_iou ---------------------------------------------------------------------------------------------------
def test_axis_aligned_boxes_agree_with_get_iou():
    rng = np.random.default_rng(2)
    n = 600
    ctr = rng.integers(-64, 65, (n, 3)) / 64.0
    ext = rng.integers(0, 129, (n, 3)) / 64.0                  # (zero extents occur)
    obb = np.concatenate([ctr, ext, np.zeros((n, 1))], axis=1)
    six = np.concatenate([ctr - 0.5 * ext, ctr + 0.5 * ext], axis=1)     # exact: multiples of 1/128
    rows = BX.boxes8(obb)
    assert (rows[:, 6] == 1).all() and (rows[:, 7] == 0).all()
    zeros = positive = 0
    for i in range(0, n, 2):
        want = get_iou(six[i], six[i + 1])
        got = BX.obb_iou_pair(rows[i], rows[i + 1], '3d')
        if want == 0:
            assert got == 0.0
            zeros += 1
        else:
            assert abs(got - want) <= 1e-12, (got, want)
            positive += 1
    assert zeros >= 20 and positive >= 20


# ---- 3. invariants --------------------------------------------------------------------------------------------------------
def test_invariants():
    obb = C.random_obb(3, 20000)
    rows = BX.boxes8(obb)
    for mode in MODES:
        m = BX._mode(mode)
        own = BX._iou_rows(rows, rows, m)
        print(mode, 'worst |iou(a, a) - 1| =', np.abs(own - 1).max())
        assert np.abs(own - 1).max() <= 1e-12
        a, b = rows[:10000], rows[10000:]
        ab, ba = BX._iou_rows(a, b, m), BX._iou_rows(b, a, m)
        assert (ab > 0).mean() > 0.05
        print(mode, 'worst |iou(a, b) - iou(b, a)| =', np.abs(ab - ba).max())
        assert np.abs(ab - ba).max() <= 1e-12
        assert ((ab == 0) == (ba == 0)).mean() > 0.999          # (a touching pair may differ at the last bit)
        turned = a.copy()                                        # (du, dv, c, s) -> (dv, du, -s, c): the same rectangle
        turned[:, 3], turned[:, 4], turned[:, 6], turned[:, 7] = a[:, 4], a[:, 3], -a[:, 7], a[:, 6]
        assert np.abs(BX._iou_rows(turned, b, m) - ab).max() <= 1e-12
        assert np.abs(BX._iou_rows(b, turned, m) - ab).max() <= 1e-12


def test_octagon():
    sq = BX.boxes8(np.array([[0, 0, 0, 1, 1, 1, 0], [0, 0, 0, 1, 1, 1, np.pi / 4]], dtype=np.float64))
    assert len(BX._clip_pair(sq[0], sq[1])) == 8 and len(BX._clip_pair(sq[1], sq[0])) == 8
    area = 2 * (np.sqrt(2.0) - 1)
    assert abs(BX._area_pair(sq[0], sq[1]) - area) <= 1e-12
    assert abs(BX.obb_iou_pair(sq[0], sq[1], 'bev') - area / (2 - area)) <= 1e-12
    assert abs(BX.obb_iou_pair(sq[0], sq[1], '3d') - area / (2 - area)) <= 1e-12


# ---- 4. the degenerate list -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', C.DEGENERATE, ids=[d[0] for d in C.DEGENERATE])
def test_degenerate_list(case):
    name, a, b, want = case
    a, b = BX.boxes8(np.array([a], dtype=np.float64))[0], BX.boxes8(np.array([b], dtype=np.float64))[0]
    for x, y in ((a, b), (b, a)):
        got = BX.obb_iou_pair(x, y, '3d')
        if want is None:
            assert 0 < got <= 1 + 1e-12
        elif want == 0.0:
            assert got == 0.0 and np.signbit(got) == 0
        else:
            assert abs(got - want) <= 1e-12
    if name == 'identical':
        assert abs(BX.obb_iou_pair(a, b, '3d') - 1) <= 1e-12 and abs(BX.obb_iou_pair(a, b, 'bev') - 1) <= 1e-12
    if name in ('z_touch', 'z_apart', 'zero_dz'):                # the z rule does not exist in the bird's-eye view
        assert BX.obb_iou_pair(a, b, 'bev') > (0.5 if name == 'zero_dz' else 0.99)
    if name in ('shared_edge', 'shared_corner', 'zero_du', 'zero_dv', 'far_apart'):
        assert BX.obb_iou_pair(a, b, 'bev') == 0.0


def test_invalid_boxes_raise_and_empty_lists_do_not():
    good, bad = C.invalid_rows()
    for rows in bad:
        for mode in MODES:
            with pytest.raises(ValueError):
                BX.box_iou_numpy(rows, good, mode)
            with pytest.raises(ValueError):
                BX.box_iou_numpy(good, rows, mode)
            with pytest.raises(ValueError):
                BX.obb_iou_pair(good[0], rows[1], mode)
        with pytest.raises(ValueError):
            BX.box_nms_numpy(rows, np.ones(4), np.zeros(4, np.int32))
    with pytest.raises(ValueError):
        BX.box_iou_numpy(good, good, 'xy')
    with pytest.raises(ValueError):
        BX.box_iou_numpy(good[:, :7], good)
    none = np.zeros((0, 8))
    for mode in MODES:
        assert BX.box_iou_numpy(none, good, mode).shape == (0, 4)
        assert BX.box_iou_numpy(good, none, mode).shape == (4, 0)
        assert BX.box_iou_numpy(none, none, mode).shape == (0, 0)
    keep, n_keep, iou = BX.box_nms_numpy(none, np.zeros(0), None, return_iou=True)
    assert keep.shape == (0,) and n_keep == 0 and iou.shape == (0, 0)
    assert BX.boxes8(np.zeros((0, 7))).shape == (0, 8)


# ---- 5. the vectorised twin equals the scalar definition ------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_twin_equals_scalar_definition(mode):
    da, db = C.degenerate_rows()
    ra, rb = BX.boxes8(C.random_obb(21, 2000)), BX.boxes8(C.random_obb(22, 2000))
    ea = np.array([C.to_float(a) for a, _ in C.exact_pairs(23, 300)])
    eb = np.array([C.to_float(b) for _, b in C.exact_pairs(23, 300)])
    a, b = np.concatenate([da, db, ra, ea]), np.concatenate([db, da, rb, eb])
    got = BX._iou_rows(a, b, BX._mode(mode))
    want = np.array([BX.obb_iou_pair(x, y, mode) for x, y in zip(a, b)])
    assert (want > 0).sum() > 300
    assert np.array_equal(bits(got), bits(want))
    small = np.concatenate([da, ra[:40]]), np.concatenate([db, rb[:30]])
    mat = BX.box_iou_numpy(small[0], small[1], mode)
    loop = np.array([[BX.obb_iou_pair(x, y, mode) for y in small[1]] for x in small[0]])
    assert np.array_equal(bits(mat), bits(loop))
    assert np.array_equal(bits(BX.box_iou(small[0], small[1], mode)), bits(loop))     # numpy in, numpy out


def test_boxes8_and_get_iou_functions():
    obb = C.random_obb(4, 6)
    rows = BX.boxes8(obb)
    assert rows.shape == (6, 8) and np.array_equal(rows[:, :6], obb[:, :6])
    assert np.array_equal(rows[:, 6], np.cos(obb[:, 6])) and np.array_equal(rows[:, 7], np.sin(obb[:, 6]))
    assert np.array_equal(BX.boxes8(ObjectTable(obb=obb)), rows)
    assert get_iou_obb(obb[0], obb[1]) == BX.obb_iou_pair(rows[0], rows[1], '3d')
    assert get_iou_bev(obb[0], obb[1]) == BX.obb_iou_pair(rows[0], rows[1], 'bev')
    assert BX.auto_backend('numpy') == 'numpy' and set(BX._AUTO) == {'iou', 'nms', 'match'}


# ---- 6. the NMS twin ------------------------------------------------------------------------------------------------------
def _nms_case(seed, n, n_labels, ties):
    rng = np.random.default_rng(seed)
    obb = C.random_obb(seed, n, spread=1.5)
    obb[n // 2:n // 2 + n // 4] = obb[:n // 4] + rng.normal(0, 0.05, (n // 4, 7))      # near duplicates
    scores = rng.uniform(0.1, 1.0, n)
    if ties:
        scores = np.round(scores, 1)
        scores[:4] = [0.0, -0.0, 0.0, -0.0]
    return BX.boxes8(obb), scores, rng.integers(0, n_labels, n).astype(np.int32)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('n_labels,agnostic,ties', [(1, False, False), (4, False, True), (4, True, True)])
def test_nms_twin_against_double_loop(mode, n_labels, agnostic, ties):
    rows, scores, labels = _nms_case(31 + n_labels, 60, n_labels, ties)
    for thr in (0.1, 0.5):
        keep, n_keep, iou = BX.box_nms_numpy(rows, scores, labels, thr, mode, agnostic, return_iou=True)
        want = C.nms_loop(rows, scores, labels, thr, mode, agnostic)
        assert np.array_equal(keep, want) and n_keep == int(want.sum()) and 0 < n_keep < len(rows)
        lean = BX.box_nms_numpy(rows, scores, labels, thr, mode, agnostic)
        assert np.array_equal(lean[0], want) and lean[2] is None
        i, j = np.triu_indices(len(rows))
        assert np.array_equal(bits(iou[i, j]), bits([BX.obb_iou_pair(rows[a], rows[b], mode) for a, b in zip(i, j)]))
        assert np.array_equal(bits(iou), bits(iou.T))


def test_nms_threshold_equal_to_an_iou_does_not_suppress():
    rows = BX.boxes8(np.array([[0, 0, 0, 4, 1, 1, 0], [0, 0, 0, 1, 4, 1, 0]], dtype=np.float64))
    exact = BX.obb_iou_pair(rows[0], rows[1])
    assert exact > 0
    assert BX.box_nms_numpy(rows, [0.9, 0.8], thr=exact)[1] == 2
    assert BX.box_nms_numpy(rows, [0.9, 0.8], thr=np.nextafter(exact, 0))[1] == 1
    # equal scores: the lower index is visited first; -0.0 equals 0.0
    assert list(BX.box_nms_numpy(rows, [0.0, -0.0], thr=0.01)[0]) == [1, 0]
    assert list(BX.box_nms_numpy(rows, [-0.0, 0.0], thr=0.01)[0]) == [1, 0]
    assert list(BX.box_nms_numpy(rows, [0.1, 0.2], thr=0.01)[0]) == [0, 1]
    assert list(BX.box_nms_numpy(rows, [0.1, 0.2], [0, 1], thr=0.01)[0]) == [1, 1]
    assert list(BX.box_nms_numpy(rows, [0.1, 0.2], [0, 1], thr=0.01, class_agnostic=True)[0]) == [0, 1]
    with pytest.raises(ValueError):
        BX.box_nms_numpy(rows, [0.1, np.nan])


def test_nms_boxes_on_a_table():
    obb = C.random_obb(41, 30, spread=1.0)
    obb[[3, 17]] = np.nan                                          # empty masks: NaN boxes
    npoint = np.full(30, 10, np.int32)
    npoint[[3, 17]] = 0
    rng = np.random.default_rng(41)
    table = ObjectTable(obb=obb, npoint=npoint, conf=rng.uniform(0.1, 1, 30), label_id=rng.integers(1, 3, 30))
    keep = nms_boxes(table, 0.1, backend='numpy')
    assert keep.dtype == bool and keep.shape == (30,) and not keep[3] and not keep[17] and 0 < keep.sum() < 28
    some = np.flatnonzero(npoint)
    want = C.nms_loop(BX.boxes8(obb[some]), table['conf'][some], table['label_id'][some], 0.1, '3d', False)
    assert np.array_equal(keep[some], want != 0)
    assert np.array_equal(nms_boxes(table, 0.1), keep)             # 'auto': numpy without a GPU; the same flags with one
    small = take_rows(table, keep)
    assert isinstance(small, ObjectTable) and all(len(small[k]) == keep.sum() for k in table)
    insts = [dict(k=k) for k in range(30)]
    left, tab = nms_objects(insts, table, 0.1, backend='numpy')
    assert [i['k'] for i in left] == list(np.flatnonzero(keep)) and np.array_equal(tab['conf'], small['conf'])
    agn = nms_boxes(table, 0.1, class_agnostic=True, backend='numpy')
    assert agn.sum() <= keep.sum()
    table['obb'][5, 3] = -1.0
    with pytest.raises(ValueError):
        nms_boxes(table, 0.1, backend='numpy')


# ---- 7. matching ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('func', [get_iou_obb, get_iou_bev], ids=['3d', 'bev'])
def test_matching_numpy_path_equals_reference_loop(func, monkeypatch):
    for seed in (1, 2):
        pred, gt = C.detection_set(seed)
        job = de._ClassJob(pred, gt)
        assert job.boxes7() and job.boxes6() is None
        assert len(set(job.confidence)) < job.nd                   # equal confidences
        for t in (0.25, 0.5, 0.999):
            want = [job.finish(f, False) for f in de._match_reference_loop(job, [t], func)][0]
            got = eval_det_cls(pred, gt, t, get_iou_func=func, device='cpu')
            for g, w in zip(got, want):
                assert np.array_equal(g, w)
            assert 0 < got[2] < 1 or t == 0.999
    # the numpy path is the one that ran: the scalar function is never called
    monkeypatch.setattr(BX, 'obb_iou_pair', None)
    eval_det_cls(pred, gt, 0.25, get_iou_func=func, device='cpu')


def test_matching_other_functions_go_where_they_went():
    pred, gt = C.detection_set(3)
    calls = []

    def mine(a, b):
        calls.append(1)
        return get_iou_obb(a, b)

    got = eval_det_cls(pred, gt, 0.25, get_iou_func=mine, device='cpu')
    want = eval_det_cls(pred, gt, 0.25, get_iou_func=get_iou_obb, device='cpu')
    assert calls and all(np.array_equal(g, w) for g, w in zip(got, want))


# ---- 8. oriented AP against axis-aligned AP -------------------------------------------------------------------------------
def test_oriented_ap_with_one_yaw_step_equals_axis_aligned_ap(monkeypatch):
    s = C.synthetic_scan(n_points=6000, n_masks=24)
    args = ([s['preds']], [s['coords']], [s['semantic']], [s['instance']], s['class_labels'])
    ths = (0.25, 0.5)
    flags = {}
    real = de._ClassJob.finish

    def finish(self, tp_flags, use_07_metric):
        flags.setdefault(kind, []).append(np.array(tp_flags))
        return real(self, tp_flags, use_07_metric)

    monkeypatch.setattr(de._ClassJob, 'finish', finish)
    # precondition: no axis-aligned IoU within 1e-9 of a threshold, so that a near-tie cannot decide the outcome
    pboxes, gts = de.instance_boxes(args[1], [[p['pred_mask'] for p in s['preds']]], args[3], device='cpu')
    ious = np.array([get_iou(p, g) for p in pboxes[0] for g in gts[0][0]])
    assert (ious > 0.5).sum() >= 5 and all(np.abs(ious - t).min() > 1e-9 for t in ths)
    kind = 'aabb'
    want = evaluate_box_ap(*args, iou_thresholds=ths, device='cpu')
    kind = 'obb'
    got = evaluate_box_ap(*args, iou_thresholds=ths, device='cpu', boxes='obb', yaw_steps=1, backend='numpy')
    assert len(flags['aabb']) == len(flags['obb']) > 0
    assert all(np.array_equal(a, b) for a, b in zip(flags['aabb'], flags['obb']))
    assert sum(int(f.sum()) for f in flags['aabb']) >= 5
    for t in ths:
        assert list(got[t]['ap']) == list(want[t]['ap'])
        for c in want[t]['ap']:
            assert np.array_equal(got[t]['ap'][c], want[t]['ap'][c]) and np.array_equal(got[t]['rec'][c], want[t]['rec'][c])
        assert got[t]['mAP'] == want[t]['mAP'] > 0
    # the default argument runs today's code; the bird's-eye view can only score higher; a rotated sweep still runs
    bev = evaluate_box_ap(*args, iou_thresholds=ths, device='cpu', boxes='obb', mode='bev', yaw_steps=1,
                          backend='numpy')
    assert bev[0.5]['mAP'] >= got[0.5]['mAP']
    full = evaluate_box_ap(*args, iou_thresholds=ths, device='cpu', boxes='obb', yaw_steps=30, refine=1,
                           backend='numpy')
    assert 0 < full[0.25]['mAP'] <= 1
    with pytest.raises(ValueError):
        evaluate_box_ap(*args, boxes='sphere')


def test_oriented_instance_boxes_owners_and_errors():
    s = C.synthetic_scan(n_points=3000, n_masks=6)
    masks = [[p['pred_mask'] for p in s['preds']]]
    pb, gts = de.oriented_instance_boxes([s['coords']], masks, [s['instance']], yaw_steps=1, backend='numpy')
    ab, agts = de.instance_boxes([s['coords']], masks, [s['instance']], device='cpu')
    assert pb[0].shape == (6, 7) and gts[0][0].shape == (len(agts[0][1]), 7)
    assert np.array_equal(gts[0][1], agts[0][1]) and np.array_equal(gts[0][2], agts[0][2])       # counts, first points
    assert np.allclose(pb[0][:, :3] - 0.5 * pb[0][:, 3:6], ab[0][:, :3], atol=1e-6)
    inst = s['instance'].copy()
    inst[inst == 1] = 0                                              # owner 1 is empty
    with pytest.raises(IndexError):
        evaluate_box_ap([s['preds']], [s['coords']], [s['semantic']], [inst], s['class_labels'], device='cpu',
                        boxes='obb', backend='numpy')
    empty = [[np.zeros(len(inst), bool)]]
    with pytest.raises(ValueError):
        de.oriented_instance_boxes([s['coords']], empty, [s['instance']], backend='numpy')


# ---- 9. ranges ------------------------------------------------------------------------------------------------------------
def _const(src, name):
    m = re.search(r'constexpr\s+int\s+' + name + r'\s*=\s*(\d+)\s*;', src)
    assert m, f'constexpr int {name} not found'
    return int(m.group(1))


def test_gpu_sizes_sit_on_their_side_of_the_caps():
    with open(os.path.join(ROOT, 'softgroup_amd', 'csrc', 'box_ops.hip')) as f:
        src = f.read()
    assert G.pytestmark.name == 'gpu'
    block, grid = _const(src, 'kBoxBlock'), _const(src, 'kBoxMaxGrid')
    assert re.search(r'box_pairs_kernel<<<grid_for\(n_pairs, kBoxBlock, kBoxMaxGrid\), kBoxBlock,', src)
    assert re.search(r'box_decide_kernel<<<grid_for\(static_cast<int64_t>\(n\) \* n, kBoxBlock, kBoxMaxGrid\), kBoxBlock,', src)
    assert block * grid == G.PAIR_CAP
    na, nb = G.ABOVE_CAP
    assert G.PAIR_CAP < na * nb <= 2 * G.PAIR_CAP                   # the stride loop's second trip, and no more
    assert max(G.IOU_SIZES) ** 2 < G.PAIR_CAP                       # the other matrices take one trip
    assert _const(src, 'kBoxMaxNms') == BX.MAX_NMS_BOXES == G.NMS_MAX == 16384
    assert 1 << _const(src, 'kBoxMaxPairsLog2') == BX.MAX_PAIRS
    assert max(G.NMS_SIZES) ** 2 < G.PAIR_CAP < G.NMS_MAX ** 2      # 1000 boxes: one trip; 16 384: many
    assert _const(src, 'kBoxSlots') == 8
