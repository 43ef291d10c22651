"""Greedy mask NMS on the device: ``sg_mask_nms`` / ``sg_mask_bits_from_runs`` through ctypes, the Python surface
and the model's three ``get_instances`` paths plus ``ScanForward``, all against the brute-force loop of
tests/test_mask_nms.py on dense bool masks.  Equality everywhere; the reference has no NMS step."""
import os
import sys

import numpy as np
import pytest
import torch

from softgroup_amd import _lib as L
from softgroup_amd import ops, synthetic
from softgroup_amd.ops import nms as MN
from softgroup_amd.util import nms as UN
from softgroup_amd.util import nms_instances, rle_decode

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_mask_nms import HAND, MODES, SHAPES, SMALL, THR, bits_of, brute, case, instance_list, reference  # noqa: E402

pytestmark = pytest.mark.gpu

_MEASURE = {'iou': 0, 'min': 1}


def run_kernel(bits, N, scores, labels, thr, measure, agnostic, want_inter=True):
    """sg_mask_nms through ctypes on host arrays -> (keep, n_keep, inter | None) as numpy"""
    lib = L.lib()
    n = bits.shape[0]
    dev = torch.device('cuda')
    d_bits = torch.from_numpy(np.array(bits)).to(dev)
    d_scores = torch.from_numpy(np.array(scores, dtype=np.float32)).to(dev)
    d_labels = None if labels is None else torch.from_numpy(np.array(labels, dtype=np.int32)).to(dev)
    keep = torch.full((max(n, 1), ), 7, dtype=torch.uint8, device=dev)
    n_keep = torch.full((1, ), -1, dtype=torch.int32, device=dev)
    inter = torch.full((max(n, 1), max(n, 1)), -1, dtype=torch.int32, device=dev) if want_inter else None
    nb = lib.sg_mask_nms_workspace_bytes(n, N)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    L.check(lib.sg_mask_nms(d_bits.data_ptr() if d_bits.numel() else None, n, N, L.ptr(d_scores), L.ptr(d_labels),
                            float(thr), _MEASURE[measure], int(agnostic), L.ptr(keep), L.ptr(n_keep), L.ptr(inter),
                            L.ptr(ws), nb, L.stream()), 'sg_mask_nms')
    torch.cuda.synchronize()
    return (keep[:n].cpu().numpy(), int(n_keep.item()),
            inter[:n, :n].cpu().numpy() if want_inter and n else None)


@pytest.mark.parametrize('agnostic,measure', MODES)
@pytest.mark.parametrize('n,N', SMALL + SHAPES)
def test_kernel_equals_brute_force(n, N, agnostic, measure):
    m, s, lab, inter, keep = reference(n, N, measure, agnostic)
    if (n, N) in SHAPES:
        assert 0.10 <= 1.0 - keep.mean() <= 0.95
    got, n_keep, got_inter = run_kernel(bits_of(m), N, s, lab, THR, measure, agnostic)
    assert np.array_equal(got, keep) and n_keep == int(keep.sum())
    assert np.array_equal(got_inter, inter)
    # without the intersection matrix the pair pass may skip tile pairs: same decisions
    got2, n_keep2, _ = run_kernel(bits_of(m), N, s, lab, THR, measure, agnostic, want_inter=False)
    assert np.array_equal(got2, keep) and n_keep2 == n_keep


def test_kernel_ignores_bits_beyond_n_points():
    n, N = 67, 2049
    m, s, lab, inter, keep = reference(n, N, 'iou', False)
    bits = bits_of(m).copy()
    bits[:, -1] |= np.int32(-1) << np.int32(N % 32)
    got, n_keep, got_inter = run_kernel(bits, N, s, lab, THR, 'iou', False)
    assert np.array_equal(got, keep) and n_keep == int(keep.sum()) and np.array_equal(got_inter, inter)


@pytest.mark.parametrize('measure', ['iou', 'min'])
def test_kernel_null_labels_is_class_agnostic(measure):
    n, N = 300, 4097
    m, s, lab, inter, keep = reference(n, N, measure, True)
    assert not np.array_equal(keep, reference(n, N, measure, False)[4])
    got, n_keep, got_inter = run_kernel(bits_of(m), N, s, None, THR, measure, False)
    assert np.array_equal(got, keep) and n_keep == int(keep.sum()) and np.array_equal(got_inter, inter)


@pytest.mark.parametrize('agnostic,measure', MODES)
def test_kernel_one_mask_covers_every_point(agnostic, measure):
    n, N = 67, 2049
    m, s, lab, _ = case(n, N)
    m, s = m.copy(), s.copy()
    m[5] = True
    s[5] = 2.0                                      # visited first: with 'min' it suppresses every non-empty mask of its class
    keep, inter = brute(m, s, lab, THR, measure, agnostic)
    assert keep[5] == 1 and 0 < keep.sum() < n
    got, n_keep, got_inter = run_kernel(bits_of(m), N, s, lab, THR, measure, agnostic)
    assert np.array_equal(got, keep) and n_keep == int(keep.sum()) and np.array_equal(got_inter, inter)


@pytest.mark.parametrize('name', sorted(HAND))
def test_kernel_hand_made_cases(name):
    m, s, lab, thr, measure, want = HAND[name]
    got, n_keep, _ = run_kernel(bits_of(m), m.shape[1], np.array(s, np.float32), np.array(lab, np.int32), thr,
                                measure, False)
    assert got.tolist() == want and n_keep == sum(want)


def test_kernel_no_masks_and_range():
    lib = L.lib()
    got, n_keep, _ = run_kernel(np.zeros((0, 2), np.int32), 40, np.zeros(0, np.float32), None, THR, 'iou', True)
    assert got.size == 0 and n_keep == 0
    assert lib.sg_mask_nms_workspace_bytes(16385, 100) == 0 and lib.sg_mask_nms_workspace_bytes(4, 2 ** 31) == 0
    assert lib.sg_mask_nms_workspace_bytes(16384, 2 ** 31 - 1) > 0
    one = torch.zeros(1, dtype=torch.int32, device='cuda')
    rc = lib.sg_mask_nms(one.data_ptr(), 16385, 32, one.data_ptr(), None, 0.5, 0, 1, one.data_ptr(), one.data_ptr(),
                         None, one.data_ptr(), 4, L.stream())
    assert rc != 0 and b'range' in lib.sg_last_error()


def test_bits_from_runs_equals_packbits():
    N = 200
    sets = [list(range(0, 32)), list(range(32, 64)) + list(range(96, 128)), [], list(range(31, 33)) + [199],
            list(range(64, 200)), list(range(0, 200)), [63, 64], list(range(160, 192))]
    m = np.zeros((len(sets), N), bool)
    for k, pts in enumerate(sets):
        m[k, pts] = True
    starts, ends, bounds = [], [], [0]
    for row in m:
        d = np.diff(np.concatenate([[0], row.astype(np.int8), [0]]))
        starts += np.flatnonzero(d == 1).tolist()
        ends += np.flatnonzero(d == -1).tolist()
        bounds.append(len(starts))
    dev = torch.device('cuda')
    bits = ops.mask_bits_from_runs(torch.tensor(starts, dtype=torch.int32, device=dev),
                                   torch.tensor(ends, dtype=torch.int32, device=dev),
                                   torch.tensor(bounds, dtype=torch.int64, device=dev), N)
    assert bits.is_cuda and bits.dtype == torch.int32 and tuple(bits.shape) == (len(sets), 7)
    want = np.packbits(np.pad(m, ((0, 0), (0, 7 * 32 - N))), axis=1, bitorder='little').view(np.int32)
    assert np.array_equal(bits.cpu().numpy(), want)


# ---- Python surface ---------------------------------------------------------------------------------------------
def test_ops_mask_nms_returns_cuda_tensors():
    n, N = 130, 70001
    m, s, lab, inter, keep = reference(n, N, 'min', False)
    d = torch.from_numpy(bits_of(m)).cuda()
    k, nk, it = ops.mask_nms(d, N, torch.from_numpy(s.copy()).cuda(), torch.from_numpy(lab.copy()).cuda(), thr=THR,
                             measure='min', return_inter=True)
    assert k.is_cuda and nk.is_cuda and it.is_cuda
    assert k.dtype == torch.uint8 and nk.dtype == torch.int32 and it.dtype == torch.int32
    assert np.array_equal(k.cpu().numpy(), keep) and int(nk) == keep.sum() and np.array_equal(it.cpu().numpy(), inter)
    k2, nk2 = ops.mask_nms(d, N, torch.from_numpy(s.copy()).cuda(), None, thr=THR, class_agnostic=True)
    assert np.array_equal(k2.cpu().numpy(), reference(n, N, 'iou', True)[4])


def _device_only(monkeypatch):
    """make the host backend an error: the device path must carry these inputs"""
    def boom(*a, **k):
        raise AssertionError('host path taken')
    monkeypatch.setattr(MN, 'mask_nms_numpy', boom)
    monkeypatch.setattr(UN, '_keep_numpy', boom)


@pytest.mark.parametrize('rle', [True, False], ids=['rle', 'bool'])
@pytest.mark.parametrize('agnostic,measure', MODES)
def test_nms_instances_device_equals_numpy(rle, agnostic, measure, monkeypatch):
    n, N = 300, 4097
    m, s, lab, _, keep = reference(n, N, measure, agnostic)
    insts = instance_list(m, s, lab, rle)
    host = nms_instances(insts, THR, measure, agnostic, backend='numpy')
    assert [id(a) for a in host] == [id(insts[k]) for k in np.flatnonzero(keep)]
    _device_only(monkeypatch)
    dev = nms_instances(insts, THR, measure, agnostic, backend='device')
    assert [id(a) for a in dev] == [id(a) for a in host]


def test_nms_instances_device_rejects_unsorted_runs():
    insts = [dict(label_id=1, conf=0.5, pred_mask=dict(length=64, counts='40 3 2 5'))]
    assert len(nms_instances(insts, backend='numpy')) == 1
    with pytest.raises(ValueError):
        nms_instances(insts, backend='device')


# ---- the model ---------------------------------------------------------------------------------------------------
NMS = dict(thr=0.5, measure='iou', class_agnostic=True)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x['label_id'] == y['label_id'] and x['conf'] == y['conf'] and x['pred_mask'] == y['pred_mask']


@pytest.fixture(scope='module')
def scene():
    xyz, rgb, inst = synthetic.scene_s2(seed=5, n=20000, room_scale=0.37)
    return synthetic.make_batch(xyz, rgb, instance_labels=inst)


def _run(model, batch, tasks, nms, scan_forward=True, native=True):
    cfg = dict(synthetic.SCANNET_MODEL_CFG['test_cfg'], eval_tasks=tasks, panoptic_skip_iou=0.5)
    if nms != 'absent':
        cfg['nms'] = nms
    model.test_cfg = cfg
    model.use_scan_forward, model.use_native_scan = scan_forward, native
    with torch.no_grad():
        ret = model(batch)
    return {k: ret[k] for k in ('pred_instances', 'panoptic_preds') if k in ret}


def _brute_filter(plain):
    m = np.stack([rle_decode(p['pred_mask']) for p in plain]).astype(bool)
    keep, _ = brute(m, np.array([p['conf'] for p in plain], np.float32),
                    np.array([p['label_id'] for p in plain], np.int32), NMS['thr'], NMS['measure'],
                    NMS['class_agnostic'])
    assert 1 <= keep.sum() < len(plain), 'the scene must have duplicates to remove and something to keep'
    return [plain[k] for k in np.flatnonzero(keep)]


def test_model_paths_filter_alike(scene):
    """Every path returns exactly what the brute force leaves of that path's own unfiltered list, and the paths
    agree with each other as they do without NMS: the staged native path and the per-operator path bit for bit,
    the one-call path with the same instances and masks and confidences within 1e-5 (its class / IoU heads are FMA
    chains where the staged path calls a GEMM library: tests/test_scan_forward_gpu.py's bound, not one of NMS)."""
    model = synthetic.build_model(seed=0)
    tasks = ['semantic', 'instance']
    plain = _run(model, scene, tasks, 'absent')['pred_instances']
    _same(_run(model, scene, tasks, None)['pred_instances'], plain)
    one_call = _run(model, scene, tasks, NMS)['pred_instances']
    assert getattr(model.__dict__.get('_scan_forward'), 'last', None) is not None, 'the one-call path must have run'
    _same(one_call, _brute_filter(plain))
    plain_staged = _run(model, scene, tasks, 'absent', scan_forward=False)['pred_instances']
    _same(_run(model, scene, tasks, None, scan_forward=False)['pred_instances'], plain_staged)
    staged = _run(model, scene, tasks, NMS, scan_forward=False)['pred_instances']
    _same(staged, _brute_filter(plain_staged))
    per_op = _run(model, scene, tasks, NMS, scan_forward=False, native=False)['pred_instances']
    _same(per_op, staged)
    assert len(one_call) == len(staged)
    for x, y in zip(one_call, staged):
        assert x['label_id'] == y['label_id'] and x['pred_mask'] == y['pred_mask']
        assert abs(float(x['conf']) - float(y['conf'])) <= 1e-5


@pytest.mark.parametrize('native', [True, False], ids=['device_fusion', 'host_fusion'])
def test_model_panoptic_sees_unfiltered_instances(scene, native):
    model = synthetic.build_model(seed=0)
    tasks = ['semantic', 'instance', 'panoptic']
    a = _run(model, scene, tasks, 'absent', native=native)
    b = _run(model, scene, tasks, NMS, native=native)
    assert np.array_equal(a['panoptic_preds'], b['panoptic_preds'])
    assert 0 < len(b['pred_instances']) < len(a['pred_instances'])
    _same(b['pred_instances'], _brute_filter(a['pred_instances']))
