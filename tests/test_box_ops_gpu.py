"""The HIP kernels of csrc/box_ops.hip and the device paths of ``box_iou``, ``box_nms``, ``nms_boxes``, the oriented
matching and ``evaluate_box_ap(boxes='obb')`` against the numpy twins of ``softgroup_amd.ops.boxes`` on the cases of
tests/box_cases.py: device equals twin byte for byte (floats compared through their uint64 views), two calls give equal
bytes.  tests/test_box_ops.py pins the sizes below to the caps in the source."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_cases as C  # noqa: E402

from softgroup_amd import _lib as L  # noqa: E402
from softgroup_amd.evaluation import det_eval as de  # noqa: E402
from softgroup_amd.evaluation import eval_det_cls, evaluate_box_ap, get_iou_bev, get_iou_obb  # noqa: E402
from softgroup_amd.ops import boxes as BX  # noqa: E402
from softgroup_amd.util import describe_instances, describe_result, nms_boxes, nms_objects  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ('3d', 'bev')
IOU_SIZES = (0, 1, 2, 63, 64, 65, 257)
PAIR_CAP = 4096 * 256                    # kBoxMaxGrid * kBoxBlock: the lanes of one trip of the pair kernels
ABOVE_CAP = (1025, 1024)                 # 1 049 600 pairs: the stride loop's second trip
NMS_SIZES = (0, 1, 31, 32, 33, 1000)
NMS_MAX = 16384
_ROWS = {}


def rows_of(n, seed):
    if (n, seed) not in _ROWS:
        r = C.mixed_rows(seed, n)
        r.setflags(write=False)
        _ROWS[(n, seed)] = r
    return _ROWS[(n, seed)]


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared inputs are read-only)


def same_bytes(got, want, key=''):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (key, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.reshape(-1).view(np.uint8 if got.itemsize == 1 else f'u{got.itemsize}')
                             != want.reshape(-1).view(np.uint8 if want.itemsize == 1 else f'u{want.itemsize}'))
        raise AssertionError((key, bad.size, bad[:5], got.reshape(-1)[bad[:5]], want.reshape(-1)[bad[:5]]))


# ---- the IoU matrix -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_iou_matrix_equals_twin(mode):
    for n_a in IOU_SIZES:
        for n_b in IOU_SIZES:
            a, b = rows_of(n_a, 1), rows_of(n_b, 2)
            want = BX.box_iou_numpy(a, b, mode)
            got, again = BX.box_iou(dev(a), dev(b), mode), BX.box_iou(dev(a), dev(b), mode)
            assert got.is_cuda and got.dtype == torch.float64
            same_bytes(got, want, (n_a, n_b))
            same_bytes(again, want, (n_a, n_b))
            if n_a >= 63 and n_b >= 63:
                assert (want > 0).mean() > 0.02 and (want == 0).mean() > 0.02


def test_degenerate_list_on_the_device():
    a, b = C.degenerate_rows()
    for mode in MODES:
        got = BX.box_iou(dev(a), dev(b), mode).cpu().numpy()
        for k, (name, _, _, want) in enumerate(C.DEGENERATE):
            assert got[k, k] == BX.obb_iou_pair(a[k], b[k], mode), name
            if want == 0.0 and mode == '3d':
                assert got[k, k] == 0.0 and not np.signbit(got[k, k]), name


def test_iou_above_the_grid_cap():
    n_a, n_b = ABOVE_CAP
    a, b = rows_of(n_a, 3), rows_of(n_b, 4)
    want = BX.box_iou_numpy(a, b, '3d')
    got = BX.box_iou(dev(a), dev(b), '3d')
    same_bytes(got, want)
    assert (want[-1] > 0).any() and (want[0] > 0).any()           # both trips hold overlapping pairs


def test_invalid_boxes_set_the_flag_and_raise():
    good, bad = C.invalid_rows()
    lib = L.lib()
    for rows in bad:
        for a, b in ((rows, good), (good, rows)):
            with pytest.raises(ValueError):
                BX.box_iou(dev(a), dev(b), '3d')
        da, db = dev(rows), dev(good)
        out = torch.empty((4, 4), dtype=torch.float64, device='cuda')
        flags = torch.zeros(1, dtype=torch.int32, device='cuda')
        L.check(lib.sg_box_iou(L.ptr(da), 4, L.ptr(db), 4, 1, L.ptr(out), L.ptr(flags), L.stream()), 'sg_box_iou')
        assert int(flags.item()) == BX.FLAG_INVALID
        keep, n_keep = BX.box_nms(da, dev(np.ones(4, np.float32)), None, 0.5)
        assert int(n_keep[1].item()) == BX.FLAG_INVALID and keep.shape == (4,)
        obb = np.concatenate([rows[:, :6], np.zeros((4, 1))], 1)
        if BX._invalid(BX.boxes8(obb)).any():                       # (the bad entry is not in the cos / sin columns)
            with pytest.raises(ValueError):
                nms_boxes(dict(obb=obb, conf=np.ones(4), label_id=np.ones(4, np.int64)), backend='device')
        with pytest.raises(ValueError):
            de.match_boxes(rows, np.zeros(4, np.int32), np.arange(4, dtype=np.int32), good, [4], [0.25], 'cuda',
                           mode='3d')
    flags = torch.zeros(1, dtype=torch.int32, device='cuda')
    ok = dev(good)
    assert lib.sg_box_iou(L.ptr(ok), 1 << 16, L.ptr(ok), 1 << 15, 0, None, L.ptr(flags), L.stream()) == -4
    assert lib.sg_box_iou(L.ptr(ok), -1, L.ptr(ok), 4, 0, None, L.ptr(flags), L.stream()) == -4
    assert lib.sg_box_iou(L.ptr(ok), 4, L.ptr(ok), 4, 2, None, L.ptr(flags), L.stream()) == -1     # mode


# ---- matching -------------------------------------------------------------------------------------------------------------
THRESHOLDS = {1: [0.25], 3: [0.25, 0.5, 0.999], 16: [round(0.05 * k, 2) for k in range(2, 18)]}


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('n_thr', sorted(THRESHOLDS))
def test_match_equals_reference_loop(mode, n_thr):
    ths = THRESHOLDS[n_thr]
    for seed, shape in ((1, (150, 12, 7)), (2, (65, 3, 1)), (3, (1, 1, 1)), (4, (0, 4, 3)), (5, (40, 2, 0))):
        det, group, rank, gt, sizes = C.match_inputs(seed, *shape)
        want_ov, want_jm, want_tp = C.match_loop(det, group, rank, gt, sizes, ths, mode)
        ov, jm, tp = de.match_boxes(det, group, rank, gt, sizes, ths, 'cuda', mode=mode)
        same_bytes(ov, want_ov, (seed, 'ovmax'))
        same_bytes(jm, want_jm, (seed, 'jmax'))
        same_bytes(tp, want_tp, (seed, 'tp'))
        if shape[0] >= 65 and shape[2]:                              # (the cases are not empty: TPs, and GT-less groups)
            assert want_tp[0].sum() >= min(3, int((sizes > 0).sum())) and (want_jm < 0).any()
            assert np.array_equal(want_jm < 0, sizes[group] == 0)


def test_eval_det_cls_device_equals_numpy():
    for func in (get_iou_obb, get_iou_bev):
        pred, gt = C.detection_set(5, n_img=4, n_gt=6, n_det=20)
        for t in (0.25, 0.5):
            want = eval_det_cls(pred, gt, t, get_iou_func=func, device='cpu')
            got = eval_det_cls(pred, gt, t, get_iou_func=func, device='cuda')
            for g, w in zip(got, want):
                assert np.array_equal(g, w)


# ---- NMS ------------------------------------------------------------------------------------------------------------------
def _nms_inputs(n, n_labels):
    rng = np.random.default_rng(100 + n)
    rows = rows_of(n, 7).copy()
    if n >= 8:
        rows[n // 2:n // 2 + n // 4] = rows[:n // 4]                # duplicates: something to suppress
    scores = np.round(rng.uniform(0.1, 1.0, n), 2).astype(np.float32)    # two decimals: equal scores occur
    if n >= 4:
        scores[:4] = [0.0, -0.0, 0.0, -0.0]
    labels = rng.integers(0, n_labels, n).astype(np.int32)
    if n >= 8:
        labels[n // 2:n // 2 + n // 4] = labels[:n // 4]
    return rows, scores, labels


@pytest.mark.parametrize('n_labels,agnostic', [(1, False), (5, False), (5, True)])
@pytest.mark.parametrize('n', NMS_SIZES)
def test_nms_equals_twin(n, n_labels, agnostic):
    rows, scores, labels = _nms_inputs(n, n_labels)
    for mode in (MODES if n == 33 else ('3d',)):
        want_keep, want_n, want_iou = BX.box_nms_numpy(rows, scores, labels, 0.3, mode, agnostic, return_iou=True)
        args = (dev(rows), dev(scores), dev(labels), 0.3, mode, agnostic)
        keep, n_keep, iou = BX.box_nms(*args, return_iou=True)
        same_bytes(keep, want_keep, 'keep')
        assert n_keep.cpu().tolist() == [want_n, 0]
        same_bytes(iou, want_iou, 'iou')
        lean, lean_n = BX.box_nms(*args)                            # without the matrix: the label and index skips
        same_bytes(lean, want_keep, 'keep, lean')
        assert lean_n.cpu().tolist() == [want_n, 0]
        if n >= 31:
            assert 0 < want_n < n


def test_nms_at_the_largest_size_and_beyond():
    n = NMS_MAX
    k = np.arange(n // 2)
    obb = np.zeros((n, 7))
    obb[0::2, 0] = obb[1::2, 0] = 10.0 * (k % 128)                  # pairs on a lattice, 10 apart, boxes < 3 across
    obb[0::2, 1] = obb[1::2, 1] = 10.0 * (k // 128)
    obb[0::2, 3:6] = obb[1::2, 3:6] = np.stack([1.0 + (k % 7) / 8, 2.0 - (k % 5) / 8, 1.0 + (k % 3) / 4], 1)
    obb[0::2, 6] = obb[1::2, 6] = 0.1 * (k % 31)
    rows = BX.boxes8(obb)
    scores = (1.0 - np.arange(n) / n).astype(np.float32)            # descending with the index
    assert (np.diff(scores) < 0).all()
    keep, n_keep = BX.box_nms(dev(rows), dev(scores), dev(np.zeros(n, np.int32)), 0.5)
    want = np.zeros(n, np.uint8)
    want[0::2] = 1                                                   # every IoU is 0, or within ulps of 1 for (2k, 2k+1)
    same_bytes(keep, want)
    assert n_keep.cpu().tolist() == [n // 2, 0]
    lib = L.lib()
    assert lib.sg_box_nms_workspace_bytes(n) > 0 and lib.sg_box_nms_workspace_bytes(n + 1) == 0
    more = dev(np.concatenate([rows, rows[:1]]))
    ws = L.workspace(lib.sg_box_nms_workspace_bytes(n), more.device)
    out, cnt = torch.empty(n + 1, dtype=torch.uint8, device='cuda'), torch.zeros(2, dtype=torch.int32, device='cuda')
    rc = lib.sg_box_nms(L.ptr(more), n + 1, L.ptr(dev(np.ones(n + 1, np.float32))), None, 0.5, 0, 1, L.ptr(out),
                        L.ptr(cnt), None, L.ptr(ws), ws.numel(), L.stream())
    assert rc == -4 and b'sg_box_nms' in lib.sg_last_error()        # SG_ERR_UNSUPPORTED
    with pytest.raises(L.SoftGroupHipError):
        BX.box_nms(more, dev(np.ones(n + 1, np.float32)))


# ---- device against numpy, end to end -------------------------------------------------------------------------------------
def test_nms_boxes_and_box_ap_device_equal_numpy():
    s = C.synthetic_scan()
    assert 15000 <= len(s['coords']) <= 25000 and len(s['preds']) == 40
    tab_n = describe_instances(s['preds'], s['coords'], backend='numpy')
    result = dict(pred_instances=s['preds'], coords_float=torch.from_numpy(s['coords']).cuda())
    tab_d = describe_result(result, backend='device')
    same_bytes(tab_d['obb'], tab_n['obb'], 'obb')
    for mode in MODES:
        for agnostic in (False, True):
            want = nms_boxes(tab_n, 0.25, mode, agnostic, backend='numpy')
            got = nms_boxes(tab_d, 0.25, mode, agnostic, backend='device')
            same_bytes(got, want, ('nms_boxes', mode, agnostic))
            assert 0 < want.sum() < 40
    left, small = nms_objects(s['preds'], tab_d, backend='device')
    assert len(left) == len(small['conf']) == nms_boxes(tab_n, backend='numpy').sum()
    args = ([s['preds']], [s['coords']], [s['semantic']], [s['instance']], s['class_labels'])
    for mode in MODES:
        want = evaluate_box_ap(*args, boxes='obb', mode=mode, yaw_steps=45, backend='numpy')
        got = evaluate_box_ap(*args, boxes='obb', mode=mode, yaw_steps=45, backend='device')
        for t in want:
            assert list(got[t]['ap']) == list(want[t]['ap']) and got[t]['mAP'] == want[t]['mAP'] > 0
            for c in want[t]['ap']:
                assert np.array_equal(got[t]['rec'][c], want[t]['rec'][c])
                assert np.array_equal(got[t]['prec'][c], want[t]['prec'][c])
