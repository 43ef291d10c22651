"""Masks and labels snapped to superpoints: the numpy twins of softgroup_amd.ops.superpoint against a brute force of
plain loops over dense arrays, the hand-made cases of the rules, and the list / result surface of
softgroup_amd.util.superpoint on the host.  The reference has no such step."""
import copy
import json
import os
import sys

import numpy as np
import pytest

from softgroup_amd import ops
from softgroup_amd.ops import superpoint as SP
from softgroup_amd.util import load_scannet_segs, refine_result, rle_decode, rle_encode, snap_instances
from softgroup_amd.util.lazy import LazyResults

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_mask_split import bits_of, dense_of, instance_list, same_lists  # noqa: E402

MODES = ('snap', 'grow', 'trim')


# ---- brute force ---------------------------------------------------------------------------------------------------
def brute_segments(sp):
    """[(id, [points ascending])] in ascending id order"""
    sp = [int(v) for v in sp]
    for v in sp:
        if v < -1 or v >= 2**31 - 1:
            raise ValueError('id')
    return [(i, [p for p in range(len(sp)) if sp[p] == i]) for i in sorted(set(sp) - {-1})]


def brute_snap(dense, sp, thr, mode):
    dense = np.asarray(dense, bool)
    out = dense.copy()
    for k in range(dense.shape[0]):
        for _, pts in brute_segments(sp):
            inter = sum(int(dense[k, p]) for p in pts)
            taken = inter >= 1 and float(inter) / float(len(pts)) > thr
            for p in pts:
                out[k, p] = taken if mode == 'snap' else (dense[k, p] or taken) if mode == 'grow' else \
                    (dense[k, p] and taken)
    return out


def brute_vote(labels, sp, n_classes, ignore_label=-100):
    out = np.array(labels).copy()
    for _, pts in brute_segments(sp):
        count = [0] * n_classes
        for p in pts:
            v = int(labels[p])
            if 0 <= v < n_classes and v != ignore_label:
                count[v] += 1
        if max(count) > 0:
            out[pts] = count.index(max(count))               # (the first of equal counts: the lowest class)
    return out


# ---- clouds --------------------------------------------------------------------------------------------------------
def make_sp(N, seed=0, sizes=(), none=0.1, ids=()):
    """int64 ids [N]: segments of ``sizes`` first, then random ones of 1 - 6 points, about ``none`` of the rest in
    no segment; ids are scattered over 0 .. 2**31 - 2 (``ids`` among them) and the points are shuffled, so a segment
    is anywhere in the cloud"""
    rng = np.random.default_rng(seed)
    sp = np.full(N, -1, np.int64)
    pos, seg = 0, 0
    for s in sizes:
        assert pos + s <= N
        sp[pos:pos + s] = seg
        pos, seg = pos + s, seg + 1
    while pos < N:
        s = min(int(rng.integers(1, 7)), N - pos)
        if rng.random() >= none:
            sp[pos:pos + s] = seg
            seg += 1
        pos += s
    names = set(int(v) for v in ids)
    while len(names) < seg:
        names.add(int(rng.integers(0, 2**31 - 1)))
    names = rng.permutation(np.array(sorted(names), np.int64)[:seg]) if seg else np.zeros(0, np.int64)
    out = np.where(sp >= 0, names[np.maximum(sp, 0)] if seg else -1, -1)
    return out[rng.permutation(N)]


def make_masks(n, sp, seed=0):
    """bool [n, N]: per mask a few segments almost whole, a few barely touched, and noise"""
    rng = np.random.default_rng(seed + 1000)
    N = sp.size
    ids = np.unique(sp[sp >= 0])
    dense = np.zeros((n, N), bool)
    for k in range(n):
        if ids.size:
            pick = rng.choice(ids, size=max(1, ids.size // 3), replace=False)
            dense[k] = np.isin(sp, pick) & (rng.random(N) < rng.choice([0.3, 0.5, 0.9]))
        dense[k] |= rng.random(N) < 0.03
    return dense


def check_index(idx, sp):
    segs = brute_segments(sp)
    assert idx.n_points == len(sp) and idx.n_seg == len(segs)
    assert idx.n_valid == sum(len(p) for _, p in segs)
    assert idx.max_size == max([len(p) for _, p in segs] + [0])
    assert idx.order.dtype == np.int32 and idx.seg_of.dtype == np.int32 and idx.seg_start.dtype == np.int32
    assert idx.order.tolist() == [p for _, pts in segs for p in pts]
    assert idx.seg_start.tolist() == np.concatenate([[0], np.cumsum([len(p) for _, p in segs])]).astype(int).tolist()
    want = np.full(len(sp), -1)
    for s, (_, pts) in enumerate(segs):
        want[pts] = s
    assert idx.seg_of.tolist() == want.tolist()


# ---- the index -----------------------------------------------------------------------------------------------------
def test_index_hand_made():
    sp = np.array([1_000_000, 7, -1, 2**31 - 2, 7, 1_000_000, 7, -1])
    idx = ops.superpoint_index(sp)
    assert isinstance(idx, ops.SuperpointIndex) and not idx.is_cuda
    check_index(idx, sp)
    assert idx.order.tolist() == [1, 4, 6, 0, 5, 3] and idx.seg_start.tolist() == [0, 3, 5, 6]
    assert idx.seg_of.tolist() == [1, 0, -1, 2, 0, 1, 0, -1] and idx.max_size == 3


@pytest.mark.parametrize('N,seed', [(1, 0), (33, 1), (200, 2), (257, 3)])
def test_index_equals_brute_force(N, seed):
    sp = make_sp(N, seed, sizes=(5, ) if N > 5 else ())
    check_index(SP.superpoint_index_numpy(sp), sp)
    check_index(SP.superpoint_index_numpy(sp.astype(np.int32)), sp)


def test_index_edge_cases():
    check_index(SP.superpoint_index_numpy(np.zeros(0, np.int64)), [])
    check_index(SP.superpoint_index_numpy(np.full(9, -1)), [-1] * 9)
    import torch
    check_index(ops.superpoint_index(torch.tensor([3, 3, -1, 0])), [3, 3, -1, 0])
    for bad in (-2, 2**31 - 1, 2**40):
        with pytest.raises(ValueError):
            SP.superpoint_index_numpy(np.array([0, bad, 1], np.int64))
    with pytest.raises(ValueError):
        SP.superpoint_index_numpy(np.zeros((2, 2), np.int64))
    with pytest.raises(ValueError):
        SP.superpoint_index_numpy(np.zeros(3, np.float32))


# ---- mask snap -----------------------------------------------------------------------------------------------------
def snap_dense(dense, sp, thr, mode):
    N = dense.shape[1]
    out_bits, npoint = SP.mask_snap_numpy(bits_of(dense), N, SP.superpoint_index_numpy(sp), thr, mode)
    assert out_bits.dtype == np.int32 and out_bits.shape == (dense.shape[0], (N + 31) // 32)
    got = dense_of(out_bits, N)
    assert npoint.dtype == np.int32 and npoint.tolist() == got.sum(1).tolist()
    assert np.array_equal(out_bits, bits_of(got)), 'the bits at and beyond N must be zero'
    return got


def test_snap_threshold_is_strict():
    sp = np.array([5, 5, 5, 5, 9])
    two = np.array([[1, 1, 0, 0, 0]], bool)
    three = np.array([[1, 1, 1, 0, 0]], bool)
    assert snap_dense(two, sp, 0.5, 'snap').tolist() == [[False] * 5]                # 2 / 4 > 0.5 is false
    assert snap_dense(three, sp, 0.5, 'snap').tolist() == [[True] * 4 + [False]]
    # thr = 0: any touched segment is taken, an untouched one is not; thr = 1: nothing is
    assert snap_dense(np.array([[0, 0, 0, 1, 0]], bool), sp, 0.0, 'snap').tolist() == [[True] * 4 + [False]]
    assert snap_dense(np.array([[1, 1, 1, 1, 1]], bool), sp, 1.0, 'snap').tolist() == [[False] * 5]


def test_snap_modes_and_free_points():
    #              seg A (3 of 4)  seg B (1 of 4)  free
    sp = np.array([4, 4, 4, 4, 2, 2, 2, 2, -1, -1])
    m = np.array([[1, 1, 1, 0, 1, 0, 0, 0, 1, 0]], bool)
    snap, grow, trim = (snap_dense(m, sp, 0.5, mode)[0] for mode in MODES)
    assert snap.astype(int).tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 1, 0]
    assert grow.astype(int).tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 1, 0]
    assert trim.astype(int).tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 1, 0]
    assert (grow >= m[0]).all() and (trim <= m[0]).all()
    assert not (snap >= m[0]).all() and not (snap <= m[0]).all()      # 'snap' is neither a superset nor a subset


def test_snap_arbitrary_ids():
    sp = np.array([2**31 - 2, 7, 1_000_000, 7, 2**31 - 2, 1_000_000, 7])
    m = np.array([[1, 1, 0, 1, 0, 0, 0], [0, 0, 1, 0, 1, 1, 0]], bool)
    for mode in MODES:
        assert np.array_equal(snap_dense(m, sp, 0.5, mode), brute_snap(m, sp, 0.5, mode))
    assert snap_dense(m, sp, 0.5, 'snap').astype(int).tolist() == [[0, 1, 0, 1, 0, 0, 1], [0, 0, 1, 0, 0, 1, 0]]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('n,N,thr', [(1, 1, 0.5), (3, 31, 0.0), (2, 33, 0.5), (4, 200, 0.5), (3, 257, 1.0),
                                     (3, 130, 0.25)])
def test_snap_equals_brute_force(n, N, thr, mode):
    sp = make_sp(N, seed=N, sizes=(40, ) if N > 100 else ())
    dense = make_masks(n, sp, seed=n)
    assert np.array_equal(snap_dense(dense, sp, thr, mode), brute_snap(dense, sp, thr, mode))


def test_snap_edge_cases():
    sp = make_sp(45, seed=4)
    idx = SP.superpoint_index_numpy(sp)
    empty = np.zeros((2, 45), bool)
    assert not snap_dense(empty, sp, 0.0, 'grow').any()
    out_bits, npoint = SP.mask_snap_numpy(np.zeros((0, 2), np.int32), 45, idx)
    assert out_bits.shape == (0, 2) and npoint.shape == (0, )
    out_bits, npoint = SP.mask_snap_numpy(np.zeros((3, 0), np.int32), 0, SP.superpoint_index_numpy(np.zeros(0, int)))
    assert out_bits.shape == (3, 0) and npoint.tolist() == [0, 0, 0]
    # bits of the input at and beyond N are ignored, those of the output are zero
    dense = make_masks(2, sp, seed=9)
    dirty = bits_of(dense).copy()
    dirty[:, -1] |= np.int32(-1) << np.int32(45 - 32)
    for mode in MODES:
        got, npoint = SP.mask_snap_numpy(dirty, 45, idx, 0.5, mode)
        assert np.array_equal(got, bits_of(brute_snap(dense, sp, 0.5, mode)))
    # tensors in, tensors out; packed bytes are rows too
    import torch
    t_bits, t_np = ops.mask_snap(torch.from_numpy(bits_of(dense)), 45, idx, 0.5, 'grow')
    assert torch.is_tensor(t_bits) and np.array_equal(t_bits.numpy(), bits_of(brute_snap(dense, sp, 0.5, 'grow')))
    b_bits, _ = SP.mask_snap_numpy(bits_of(dense).view(np.uint8), 45, idx, 0.5, 'grow')
    assert np.array_equal(b_bits, t_bits.numpy())
    for bad in (dict(thr=-0.1), dict(thr=1.5), dict(thr=float('nan')), dict(mode='shrink')):
        with pytest.raises(ValueError):
            SP.mask_snap_numpy(bits_of(dense), 45, idx, **bad)
    with pytest.raises(ValueError):
        SP.mask_snap_numpy(bits_of(dense), 45, SP.superpoint_index_numpy(sp[:44]))


# ---- label vote ----------------------------------------------------------------------------------------------------
def test_vote_hand_made():
    #              seg 3: tie 1 / 2 -> 1     seg 8: only ignored      free
    sp = np.array([3, 3, 3, 3, 3, 8, 8, -1, 3])
    lab = np.array([2, 1, 2, 1, -100, -100, 77, 2, 40], np.int16)
    idx = SP.superpoint_index_numpy(sp)
    out = ops.superpoint_vote(lab, idx, 20)
    assert out.dtype == np.int16 and out.tolist() == [1, 1, 1, 1, 1, -100, 77, 2, 1]
    assert np.array_equal(out, brute_vote(lab, sp, 20))
    # an ignore_label inside the classes is not counted either
    assert ops.superpoint_vote(lab, idx, 20, ignore_label=1).tolist() == [2, 2, 2, 2, 2, -100, 77, 2, 2]
    import torch
    t = ops.superpoint_vote(torch.from_numpy(lab.astype(np.int64)), idx, 20)
    assert t.dtype == torch.int64 and t.tolist() == out.tolist()
    u = ops.superpoint_vote(lab.astype(np.uint8), idx, 20)
    assert u.dtype == np.uint8 and np.array_equal(u, brute_vote(lab.astype(np.uint8), sp, 20))


@pytest.mark.parametrize('N,C', [(1, 1), (40, 3), (200, 20), (257, 300)])
def test_vote_equals_brute_force(N, C):
    sp = make_sp(N, seed=N + 1, sizes=(50, ) if N > 100 else ())
    rng = np.random.default_rng(N)
    lab = rng.integers(-2, C + 2, size=N)
    lab[rng.random(N) < 0.2] = -100
    out = SP.superpoint_vote_numpy(lab, SP.superpoint_index_numpy(sp), C)
    assert np.array_equal(out, brute_vote(lab, sp, C))
    with pytest.raises(ValueError):
        SP.superpoint_vote_numpy(lab, SP.superpoint_index_numpy(sp), 0)


# ---- lists and results ---------------------------------------------------------------------------------------------
def _scene(n=6, N=300, seed=5):
    sp = make_sp(N, seed=seed, sizes=(30, 20))
    dense = make_masks(n, sp, seed=seed)
    dense[n - 1] = False
    dense[n - 1, :2] = True                                   # a mask that loses everything to 'snap'
    return sp, dense


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('rle', [True, False], ids=['rle', 'dense'])
def test_snap_instances_numpy(rle, mode):
    sp, dense = _scene()
    insts = instance_list(dense, rle)
    before = copy.deepcopy(insts)
    want = brute_snap(dense, sp, 0.5, mode)
    got = snap_instances(insts, sp, 0.5, mode, backend='numpy')
    assert len(got) == len(insts)
    for k, (g, src) in enumerate(zip(got, insts)):
        assert g is not src and set(g) == {'scan_id', 'label_id', 'conf', 'pred_mask'}
        assert all(g[key] == src[key] for key in ('scan_id', 'label_id', 'conf'))
        if rle:
            assert g['pred_mask'] == rle_encode(want[k].astype(np.int32))
            assert np.array_equal(rle_decode(g['pred_mask']).astype(bool), want[k])
        else:
            assert g['pred_mask'].dtype == bool and np.array_equal(g['pred_mask'], want[k])
    for a, b in zip(insts, before):                           # the input is untouched
        assert a['label_id'] == b['label_id'] and a['conf'] == b['conf']
        assert a['pred_mask'] == b['pred_mask'] if rle else np.array_equal(a['pred_mask'], b['pred_mask'])
    # min_npoint drops instances; an index serves as well as the ids
    size = want.sum(1)
    cut = int(np.sort(size)[len(size) // 2]) + 1
    few = snap_instances(insts, ops.superpoint_index(sp), 0.5, mode, min_npoint=cut, backend='numpy')
    assert 0 < len(few) < len(insts)
    same = [g for g, s in zip(got, size) if s >= cut]
    if rle:
        same_lists(few, same)
    else:
        assert [f['conf'] for f in few] == [s['conf'] for s in same]
        assert all(np.array_equal(f['pred_mask'], s['pred_mask']) for f, s in zip(few, same))
    assert snap_instances(insts, sp, 0.5, mode, min_npoint=int(size.max()) + 1, backend='numpy') == []    # all dropped
    assert snap_instances([], sp, backend='numpy') == []
    with pytest.raises(ValueError):
        snap_instances(insts, sp[:-1], backend='numpy')
    with pytest.raises(ValueError):
        snap_instances(insts, sp, min_npoint=-1, backend='numpy')
    with pytest.raises(ValueError):
        snap_instances(insts, sp, backend='gpu')


def test_refine_result():
    sp, dense = _scene()
    N = sp.size
    rng = np.random.default_rng(0)
    sem = rng.integers(0, 5, size=N).astype(np.int64)
    sem[::7] = -100
    result = dict(scan_id='scene0000_00', semantic_preds=sem, pred_instances=instance_list(dense),
                  panoptic_preds=np.arange(N), offset_preds=np.zeros((N, 3), np.float32), coords_float=np.ones((N, 3)))
    before = copy.deepcopy(result)
    out = refine_result(result, sp, backend='numpy')
    assert out is not result and set(out) == set(result)
    for key in ('scan_id', 'panoptic_preds', 'offset_preds', 'coords_float'):
        assert out[key] is result[key]
    assert out['semantic_preds'].dtype == np.int64 and np.array_equal(out['semantic_preds'], brute_vote(sem, sp, 5))
    assert not np.array_equal(out['semantic_preds'], sem)
    same_lists(out['pred_instances'], snap_instances(result['pred_instances'], sp, backend='numpy'))
    assert np.array_equal(result['semantic_preds'], before['semantic_preds'])
    same_lists(result['pred_instances'], before['pred_instances'])
    # each part can be left alone
    a = refine_result(result, sp, masks=None, backend='numpy')
    assert a['pred_instances'] is result['pred_instances']
    assert np.array_equal(a['semantic_preds'], out['semantic_preds'])
    b = refine_result(result, ops.superpoint_index(sp), semantic=False, backend='numpy',
                      masks=dict(thr=0.3, mode='grow', min_npoint=5))
    assert b['semantic_preds'] is result['semantic_preds']
    same_lists(b['pred_instances'], snap_instances(result['pred_instances'], sp, 0.3, 'grow', 5, backend='numpy'))
    # n_classes given: labels at and above it are not counted
    c = refine_result(result, sp, masks=None, n_classes=3, backend='numpy')
    assert np.array_equal(c['semantic_preds'], brute_vote(sem, sp, 3))
    with pytest.raises(ValueError):
        refine_result(result, sp, masks=dict(radius=1.0), backend='numpy')
    # a lazy result is resolved first; a result without the keys passes through
    lazy = LazyResults(scan_id='s')
    from concurrent.futures import Future
    fut = Future()
    fut.set_result(dict(semantic_preds=sem))
    lazy.defer(fut)
    assert np.array_equal(refine_result(lazy, sp, backend='numpy')['semantic_preds'], out['semantic_preds'])
    assert refine_result(dict(scan_id='s'), sp, backend='numpy') == dict(scan_id='s')


def test_auto_backend_follows_the_table(monkeypatch):
    import torch
    assert set(SP._AUTO) == {'snap', 'vote'} and set(SP._AUTO.values()) <= {'device', 'numpy'}
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    assert SP.auto_backend('auto', 'snap') == 'numpy' and SP.auto_backend('device', 'vote') == 'device'
    with pytest.raises(ValueError):
        SP.auto_backend('gpu', 'snap')


def test_load_scannet_segs(tmp_path):
    path = tmp_path / 'scene0000_00_vh_clean_2.0.010000.segs.json'
    ids = [5, 5, 900001, 0, 5, 900001]
    path.write_text(json.dumps(dict(params=dict(kThresh='0.0001'), sceneId='scene0000_00', segIndices=ids)))
    seg = load_scannet_segs(str(path))
    assert seg.dtype == np.int32 and seg.tolist() == ids
    check_index(ops.superpoint_index(seg), ids)
    path.write_text(json.dumps(dict(segIndices=[[1, 2]])))
    with pytest.raises(ValueError):
        load_scannet_segs(str(path))
