"""Masks and labels snapped to superpoints on the device: ``sg_superpoint_index``, ``sg_mask_snap`` and
``sg_superpoint_vote`` through ctypes into poisoned buffers with spare rows behind them, and the Python surface,
against the numpy twins that tests/test_superpoint.py checks against the brute force.  Equality everywhere; the
reference has no such step.

``sg_mask_snap`` reads the taken rows from global memory in every shape (it has no second, LDS-staged path), so no
shape is needed to reach one."""
import os
import sys

import numpy as np
import pytest
import torch

from softgroup_amd import _lib as L
from softgroup_amd import ops, synthetic
from softgroup_amd.data import voxel_downsample
from softgroup_amd.ops import superpoint as SP
from softgroup_amd.util import refine_result, snap_instances
from softgroup_amd.util import superpoint as US

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_mask_split import bits_of, instance_list, same_lists  # noqa: E402
from test_superpoint import MODES, make_masks, make_sp  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
SPARE = 3
WALK = SP.WALK
_MODE = {'snap': 0, 'grow': 1, 'trim': 2}
DEV = torch.device('cuda')


def poisoned(*shape):
    return torch.full(shape, POISON, dtype=torch.int32, device=DEV)


def dirty_ws(nbytes):
    assert nbytes > 0
    return torch.full((nbytes, ), 0x5A, dtype=torch.uint8, device=DEV)


def up(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def ordered_sp(sizes, N, seed=0, none=0):
    """ids [N] whose segments, in ascending id order (the order of ``order``), have ``sizes``; ``none`` points in no
    segment and the rest in single-point segments; the points are shuffled"""
    rng = np.random.default_rng(seed)
    sp = np.full(N, -1, np.int64)
    pos = 0
    for i, s in enumerate(sizes):
        sp[pos:pos + s] = 10 * i + 3
        pos += s
    rest = N - pos - none
    assert rest >= 0
    sp[pos:pos + rest] = 10 * len(sizes) + 3 + 2 * np.arange(rest)
    return sp[rng.permutation(N)]


# ---- the kernels through ctypes ------------------------------------------------------------------------------------
def run_index(sp):
    """-> (rc, meta, order, seg_of, seg_start) as host arrays, SPARE words behind each"""
    lib = L.lib()
    N = len(sp)
    d_sp = up(sp)
    order, seg_of, seg_start = poisoned(N + SPARE), poisoned(N + SPARE), poisoned(N + 1 + SPARE)
    meta = torch.full((4, ), -77, dtype=torch.int32, device=DEV)
    nb = lib.sg_superpoint_index_workspace_bytes(N)
    ws = dirty_ws(nb)
    rc = lib.sg_superpoint_index(L.ptr(d_sp) if N else None, N, L.ptr(order), L.ptr(seg_of), L.ptr(seg_start),
                                 L.ptr(meta), L.ptr(ws), nb, L.stream())
    torch.cuda.synchronize()
    return rc, meta.cpu().tolist(), order.cpu().numpy(), seg_of.cpu().numpy(), seg_start.cpu().numpy()


def check_index(sp):
    want = SP.superpoint_index_numpy(sp)
    rc, meta, order, seg_of, seg_start = run_index(sp)
    N = len(sp)
    assert rc == 0 and meta == [want.n_seg, 0, want.n_valid, want.max_size]
    assert np.array_equal(order[:want.n_valid], want.order) and (order[want.n_valid:] == POISON).all()
    assert np.array_equal(seg_of[:N], want.seg_of) and (seg_of[N:] == POISON).all()
    assert np.array_equal(seg_start[:want.n_seg + 1], want.seg_start) and (seg_start[want.n_seg + 1:] == POISON).all()
    return want


def device_index(idx):
    """the twin's arrays on the device, in buffers of the size the kernels are promised"""
    order = poisoned(idx.n_points + 1)
    order[:idx.n_valid] = up(idx.order)
    seg_start = poisoned(idx.n_points + 1)
    seg_start[:idx.n_seg + 1] = up(idx.seg_start)
    return order, up(idx.seg_of), seg_start


def run_snap(bits, N, idx, thr, mode, d_idx=None):
    """-> (out_bits [n, W], npoint [n]); every word written, nothing behind the outputs"""
    lib = L.lib()
    n, W = bits.shape[0], (N + 31) // 32
    d_bits = up(bits)
    order, seg_of, seg_start = d_idx or device_index(idx)
    out_bits, npoint = poisoned(n + SPARE, W), poisoned(n + SPARE)
    nb = lib.sg_mask_snap_workspace_bytes(n, N, idx.n_seg)
    ws = dirty_ws(nb)
    L.check(lib.sg_mask_snap(L.ptr(d_bits), n, N, L.ptr(order), L.ptr(seg_of), L.ptr(seg_start), idx.n_seg, idx.n_valid,
                             float(thr), _MODE[mode], L.ptr(out_bits), L.ptr(npoint), L.ptr(ws), nb, L.stream()),
            'sg_mask_snap')
    torch.cuda.synchronize()
    out_bits, npoint = out_bits.cpu().numpy(), npoint.cpu().numpy()
    assert (out_bits[n:] == POISON).all() and (npoint[n:] == POISON).all(), 'written behind the outputs'
    return out_bits[:n], npoint[:n]


def check_snap(dense, sp, thrs=(0.0, 0.5, 1.0), modes=MODES, idx=None):
    N = dense.shape[1]
    idx = idx or SP.superpoint_index_numpy(sp)
    bits = bits_of(dense)
    if N % 32:
        bits = bits.copy()
        bits[:, -1] |= np.int32(-1) << np.int32(N % 32)        # the input's bits at and beyond N are ignored
    d_idx = device_index(idx)
    for thr in thrs:
        for mode in modes:
            want_bits, want_np = SP.mask_snap_numpy(bits, N, idx, thr, mode)
            got_bits, got_np = run_snap(bits, N, idx, thr, mode, d_idx)
            assert np.array_equal(got_bits, want_bits), (thr, mode)
            assert np.array_equal(got_np, want_np), (thr, mode)


def winners(labels, idx, n_classes, out):
    """the winner per segment (-1 for none) from the twin's output"""
    lab = np.asarray(labels, np.int64)
    counted = (lab >= 0) & (lab < n_classes)
    w = np.full(idx.n_seg, -1, np.int32)
    for s in range(idx.n_seg):
        pts = idx.order[idx.seg_start[s]:idx.seg_start[s + 1]]
        if counted[pts].any():
            w[s] = out[pts[0]]
    return w


def check_vote(labels, sp, n_classes, idx=None):
    lib = L.lib()
    idx = idx or SP.superpoint_index_numpy(sp)
    N = len(labels)
    want = SP.superpoint_vote_numpy(np.asarray(labels, np.int32), idx, n_classes)
    order, seg_of, seg_start = device_index(idx)
    out, seg_label = poisoned(N + SPARE), poisoned(idx.n_seg + SPARE)
    nb = lib.sg_superpoint_vote_workspace_bytes(N, idx.n_seg, n_classes)
    ws = dirty_ws(nb)
    d_lab = up(labels)
    L.check(lib.sg_superpoint_vote(L.ptr(d_lab), N, L.ptr(order), L.ptr(seg_of), L.ptr(seg_start), idx.n_seg, n_classes,
                                   -100, L.ptr(out), L.ptr(seg_label), L.ptr(ws), nb, L.stream()), 'sg_superpoint_vote')
    torch.cuda.synchronize()
    out, seg_label = out.cpu().numpy(), seg_label.cpu().numpy()
    assert np.array_equal(out[:N], want) and (out[N:] == POISON).all()
    assert np.array_equal(seg_label[:idx.n_seg], winners(labels, idx, n_classes, want))
    assert (seg_label[idx.n_seg:] == POISON).all()
    # without seg_label the winners live in the workspace: the same labels
    out2 = poisoned(N)
    L.check(lib.sg_superpoint_vote(L.ptr(d_lab), N, L.ptr(order), L.ptr(seg_of), L.ptr(seg_start), idx.n_seg, n_classes,
                                   -100, L.ptr(out2), None, L.ptr(ws), nb, L.stream()), 'sg_superpoint_vote')
    assert np.array_equal(out2.cpu().numpy(), want)


def random_labels(N, C, seed):
    rng = np.random.default_rng(seed)
    lab = rng.integers(-2, C + 2, size=N).astype(np.int32)
    lab[rng.random(N) < 0.2] = -100
    return lab


SIZES = (1, 63, 64, 65, 257)


def cloud(N, seed=None):
    return make_sp(N, seed=N if seed is None else seed, sizes=SIZES if N > 1000 else ())


@pytest.mark.parametrize('N', [1, 31, 32, 33, 4097])
def test_index_equals_twin(N):
    check_index(cloud(N).astype(np.int32))
    check_index(np.full(N, -1, np.int32))
    check_index(np.full(N, 2**31 - 2, np.int32))


@pytest.mark.parametrize('n', [1, 3, 65])
@pytest.mark.parametrize('N', [1, 31, 32, 33, 4097])
def test_snap_equals_twin(N, n):
    sp = cloud(N)
    check_snap(make_masks(n, sp, seed=n), sp)


def long_cases():
    """segment sizes in `order`: segments that begin inside a tile and cross one or two boundaries, segments that
    begin and end on a boundary, and many single-point segments behind them (more segments than a tile holds)"""
    return [((100, WALK + 5, 3, 2 * WALK + 1, 7), 4 * WALK + 700, 40),
            ((WALK, 2 * WALK, 5, WALK - 5, 10, WALK + WALK // 2), 7 * WALK + 33, 0),
            ((), 2 * WALK + 77, 19)]


@pytest.mark.parametrize('case', range(3))
def test_long_segments_and_many_segments(case):
    sizes, N, none = long_cases()[case]
    sp = ordered_sp(sizes, N, seed=case, none=none)
    idx = check_index(sp.astype(np.int32))
    assert idx.max_size == max(sizes + (1, )) and idx.n_seg > WALK
    rng = np.random.default_rng(case)
    dense = rng.random((3, N)) < np.array([[0.45], [0.55], [0.02]])
    check_snap(dense, sp, thrs=(0.0, 0.5), idx=idx)
    lab = random_labels(N, 6, case)
    check_vote(lab, sp, 6, idx=idx)
    lab[np.isin(sp, [13, 33])] = -100                          # long segments without a counted label
    check_vote(lab, sp, 6, idx=idx)


def test_big_case_64_masks_over_20000_points():
    N, n = 20000, 64
    sp = make_sp(N, seed=12, sizes=SIZES + (3000, ))
    idx = check_index(sp.astype(np.int32))
    check_snap(make_masks(n, sp, seed=3), sp, thrs=(0.5, ), idx=idx)
    check_vote(random_labels(N, 20, 4), sp, 20, idx=idx)


@pytest.mark.parametrize('N,C', [(1, 1), (33, 3), (4097, 20), (4097, 256)])
def test_vote_equals_twin(N, C):
    sp = cloud(N)
    check_vote(random_labels(N, C, N + C), sp, C)
    check_vote(np.full(N, -100, np.int32), sp, C)


def test_invalid_id_sets_the_flag_and_writes_nothing():
    for bad in (-2, 2**31 - 1, -2**31):
        sp = cloud(300).astype(np.int64)
        sp[211] = bad
        rc, meta, order, seg_of, seg_start = run_index(sp.astype(np.int32))
        assert rc == 0 and meta == [0, 1, 0, 0]
        for a in (order, seg_of, seg_start):
            assert (a == POISON).all()
        with pytest.raises(ValueError):
            ops.superpoint_index(torch.from_numpy(sp).to(DEV))
    wide = torch.tensor([0, 2**40, 1], device=DEV)
    with pytest.raises(ValueError):
        ops.superpoint_index(wide)
    with pytest.raises(ValueError):
        ops.superpoint_index(torch.tensor([0, -2**40, 1], device=DEV))


def test_range_and_arguments():
    lib = L.lib()
    assert lib.sg_superpoint_index_workspace_bytes(2**31) == 0
    assert lib.sg_superpoint_index_workspace_bytes(2**20) > 0
    assert lib.sg_mask_snap_workspace_bytes(16385, 100, 10) == 0
    assert lib.sg_mask_snap_workspace_bytes(4, 2**31, 10) == 0
    assert lib.sg_mask_snap_workspace_bytes(16384, 2**20, 2**18) > 0
    assert lib.sg_superpoint_vote_workspace_bytes(2**31, 10, 20) == 0
    assert lib.sg_superpoint_vote_workspace_bytes(100, 10, 257) == 0
    assert lib.sg_superpoint_vote_workspace_bytes(100, 10, 256) > 0
    one = torch.zeros(64, dtype=torch.int32, device=DEV)
    p = one.data_ptr()
    assert lib.sg_superpoint_index(p, 2**31, p, p, p, p, p, 256, L.stream()) == -4
    assert b'range' in lib.sg_last_error()
    assert lib.sg_mask_snap(p, 16385, 32, p, p, p, 1, 1, 0.5, 0, p, p, p, 256, L.stream()) == -4
    assert lib.sg_mask_snap(p, 1, 2**31, p, p, p, 1, 1, 0.5, 0, p, p, p, 256, L.stream()) == -4
    assert lib.sg_superpoint_vote(p, 32, p, p, p, 1, 257, -100, p, p, p, 256, L.stream()) == -4
    assert lib.sg_superpoint_vote(p, 2**31, p, p, p, 1, 20, -100, p, p, p, 256, L.stream()) == -4
    other = torch.zeros(64, dtype=torch.int32, device=DEV)
    for thr, mode in ((-0.1, 0), (1.5, 0), (float('nan'), 0), (0.5, 3)):
        assert lib.sg_mask_snap(p, 1, 32, p, p, p, 1, 1, thr, mode, other.data_ptr(), p, p, 256, L.stream()) == -1
    assert lib.sg_mask_snap(p, 1, 32, p, p, p, 1, 1, 0.5, 0, p, p, p, 256, L.stream()) == -1       # out_bits is bits
    assert lib.sg_mask_snap(p, 1, 32, p, p, p, 2, 1, 0.5, 0, other.data_ptr(), p, p, 256, L.stream()) == -1
    torch.cuda.synchronize()
    assert int(one.abs().sum()) == 0 and int(other.abs().sum()) == 0      # no launch: nothing was written
    with pytest.raises(L.SoftGroupHipError):
        ops.superpoint_vote(torch.zeros(4, dtype=torch.int64, device=DEV), ops.superpoint_index(np.zeros(4, int)), 257)


def test_two_calls_give_the_same_bytes():
    sizes, N, none = long_cases()[0]
    sp = ordered_sp(sizes, N, seed=8, none=none).astype(np.int32)
    a, b = run_index(sp), run_index(sp)
    assert a[1] == b[1] and all(x.tobytes() == y.tobytes() for x, y in zip(a[2:], b[2:]))
    idx = SP.superpoint_index_numpy(sp)
    bits = bits_of(make_masks(65, sp, seed=2))
    x, y = run_snap(bits, N, idx, 0.5, 'snap'), run_snap(bits, N, idx, 0.5, 'snap')
    assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()


# ---- Python surface ------------------------------------------------------------------------------------------------
def test_ops_cuda_equals_numpy():
    N = 4097
    sp = cloud(N)
    host = ops.superpoint_index(sp)
    dev = ops.superpoint_index(torch.from_numpy(sp).to(DEV))                  # int64 ids
    assert dev.is_cuda and not host.is_cuda
    assert (dev.n_points, dev.n_seg, dev.n_valid, dev.max_size) == \
        (host.n_points, host.n_seg, host.n_valid, host.max_size)
    for a, b in zip((dev.order, dev.seg_of, dev.seg_start), (host.order, host.seg_of, host.seg_start)):
        assert a.dtype == torch.int32 and np.array_equal(a.cpu().numpy(), b)
    again = dev.numpy()
    assert np.array_equal(again.order, host.order) and dev.cuda(DEV) is dev and host.numpy() is host
    bits = bits_of(make_masks(5, sp))
    want = ops.mask_snap(bits, N, host, 0.5, 'grow')
    for index in (dev, host):                                                # (a host index is uploaded)
        got = ops.mask_snap(torch.from_numpy(bits).to(DEV), N, index, 0.5, 'grow')
        assert all(g.is_cuda and g.dtype == torch.int32 for g in got)
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    none = ops.mask_snap(torch.zeros((0, 129), dtype=torch.int32, device=DEV), N, dev)
    assert tuple(none[0].shape) == (0, 129) and none[1].numel() == 0
    for dtype in (np.int64, np.int32, np.int16, np.uint8):
        lab = random_labels(N, 20, 1).astype(dtype)
        if dtype == np.int64:
            lab[5] = 2**40                                  # an uncounted label that 32 bits do not hold
        got = ops.superpoint_vote(torch.from_numpy(lab).to(DEV), dev, 20)
        assert got.is_cuda and got.dtype == torch.from_numpy(lab).dtype
        assert np.array_equal(got.cpu().numpy(), ops.superpoint_vote(lab, host, 20))
    lab = random_labels(N, 20, 2)
    assert np.array_equal(ops.superpoint_vote(torch.from_numpy(lab).to(DEV), dev, 20, ignore_label=3).cpu().numpy(),
                          ops.superpoint_vote(lab, host, 20, ignore_label=3))
    empty = ops.superpoint_index(torch.zeros(0, dtype=torch.int32, device=DEV))
    assert (empty.n_seg, empty.n_valid, empty.order.numel(), empty.seg_start.cpu().tolist()) == (0, 0, 0, [0])


@pytest.fixture(scope='module')
def scene():
    """a synthetic.scene_s1 cloud, voxel cells of 0.1 m as superpoints, 20 masks (balls of the cloud) and labels"""
    xyz, _ = synthetic.scene_s1(seed=3, n=20000)
    sp = np.asarray(voxel_downsample(xyz, 0.1, backend='numpy')[1])
    rng = np.random.default_rng(6)
    dense = np.zeros((20, xyz.shape[0]), bool)
    for k in range(20):
        c = xyz[rng.integers(xyz.shape[0])]
        dense[k] = (((xyz - c) ** 2).sum(1) < rng.uniform(0.2, 0.6) ** 2) & (rng.random(xyz.shape[0]) < 0.8)
    dense[19] = False
    dense[19, :3] = True
    sem = (np.floor(xyz[:, 0] * 2.0).astype(np.int64) % 7)
    noise = rng.random(sem.size) < 0.15
    sem[noise] = rng.integers(0, 7, size=int(noise.sum()))
    sem[::11] = -100
    return sp, dense, sem


def _device_only(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('host path taken')
    for name in ('superpoint_index_numpy', 'mask_snap_numpy', 'superpoint_vote_numpy'):
        monkeypatch.setattr(SP, name, boom)
    monkeypatch.setattr(US, '_snap_numpy', boom)


@pytest.mark.parametrize('rle', [True, False], ids=['rle', 'dense'])
def test_snap_instances_device_equals_numpy(scene, rle, monkeypatch):
    sp, dense, _ = scene
    insts = instance_list(dense, rle)
    want = {(mode, m): snap_instances(insts, sp, 0.5, mode, min_npoint=m, backend='numpy')
            for mode in MODES for m in (0, 30)}
    assert len(want['snap', 30]) < len(insts) == len(want['snap', 0])
    assert any(a['pred_mask'] != b['pred_mask'] if rle else not np.array_equal(a['pred_mask'], b['pred_mask'])
               for a, b in zip(want['snap', 0], insts))
    _device_only(monkeypatch)
    d_sp = torch.from_numpy(sp).to(DEV)                                      # stays on the device
    for (mode, m), w in want.items():
        for ids in (d_sp, sp):
            got = snap_instances(insts, ids, 0.5, mode, min_npoint=m, backend='device')
            if rle:
                same_lists(got, w)
            else:
                assert [g['conf'] for g in got] == [x['conf'] for x in w]
                assert all(g['pred_mask'].dtype == bool and np.array_equal(g['pred_mask'], x['pred_mask'])
                           for g, x in zip(got, w))


def test_refine_result_device_equals_numpy(scene, monkeypatch):
    sp, dense, sem = scene
    result = dict(scan_id='s', semantic_preds=sem, pred_instances=instance_list(dense), panoptic_preds=np.arange(5))
    want = refine_result(result, sp, backend='numpy')
    assert not np.array_equal(want['semantic_preds'], sem)
    _device_only(monkeypatch)
    built = []
    real = SP.superpoint_index
    monkeypatch.setattr(SP, 'superpoint_index', lambda ids: built.append(1) or real(ids))
    got = refine_result(result, torch.from_numpy(sp).to(DEV), backend='device')
    assert built == [1], 'one index serves both steps'
    assert got['panoptic_preds'] is result['panoptic_preds']
    assert isinstance(got['semantic_preds'], np.ndarray) and got['semantic_preds'].dtype == sem.dtype
    assert np.array_equal(got['semantic_preds'], want['semantic_preds'])
    same_lists(got['pred_instances'], want['pred_instances'])
    d_result = dict(result, semantic_preds=torch.from_numpy(sem).to(DEV))
    got = refine_result(d_result, ops.superpoint_index(torch.from_numpy(sp).to(DEV)), backend='device', masks=None)
    assert got['semantic_preds'].is_cuda and got['pred_instances'] is result['pred_instances']
    assert np.array_equal(got['semantic_preds'].cpu().numpy(), want['semantic_preds'])


def test_unsorted_runs_and_too_many_classes(monkeypatch):
    odd = [dict(scan_id='s', label_id=1, conf=0.5, pred_mask=dict(length=8, counts='7 2 1 2'))]
    sp = np.array([0, 0, 0, 1, 1, 1, 2, 2])
    want = snap_instances(odd, sp, backend='numpy')
    assert want[0]['pred_mask']['counts'] == '1 3 7 2'
    with pytest.raises(ValueError):
        snap_instances(odd, sp, backend='device')
    monkeypatch.setitem(SP._AUTO, 'snap', 'device')            # whatever 'auto' means: such strings take numpy
    monkeypatch.setitem(SP._AUTO, 'vote', 'device')
    same_lists(snap_instances(odd, sp, backend='auto'), want)
    lab = np.array([300, 300, 2, 2, 2, 300, 7, 7])
    result = dict(semantic_preds=lab)
    with pytest.raises(L.SoftGroupHipError):
        refine_result(result, sp, backend='device')
    assert refine_result(result, sp, backend='auto')['semantic_preds'].tolist() == [300, 300, 300, 2, 2, 2, 7, 7]
