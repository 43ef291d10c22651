"""The HIP kernels of csrc/ensemble.hip and the device path of ``ensemble_results``, on the cases and against the
brute forces of tests/test_ensemble.py: device equals twin byte for byte, two calls give equal bytes."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from softgroup_amd import _lib as L
from softgroup_amd import synthetic
from softgroup_amd.ops import ensemble as EN
from softgroup_amd.ops import stitch as ST
from softgroup_amd.util import ensemble_results, rle_encode

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ensemble import (E2E_CASES, SIZE_GRID, WEIGHT_SETS, brute_mask_vote, check_e2e, e2e_case, edges_of,  # noqa: E402
                           label_case, pack, stack_case, thirty_two_members_case, unpack, vote_inputs, weights_for)

pytestmark = pytest.mark.gpu

N_EDGES = (1, 31, 32, 33, 63, 65, 2049, 70001)
K_EDGES = (1, 2, 3, 8, 32)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared inputs are read-only)


def words(rows, n_bits):
    """packed uint8 rows -> CUDA int32 [G, ceil(n_bits / 32)]"""
    rows = np.ascontiguousarray(rows)
    return dev(rows.view(np.int32).reshape(rows.shape[0], (n_bits + 31) // 32))


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def _csrc():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'softgroup_amd', 'csrc',
                        'ensemble.hip')
    with open(path) as f:
        return f.read()


def _const(src, name):
    m = re.search(r'constexpr\s+int\s+' + name + r'\s*=\s*(\d+)\s*;', src)
    assert m, f'constexpr int {name} not found'
    return int(m.group(1))


# ---- label vote -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', K_EDGES)
@pytest.mark.parametrize('n', N_EDGES)
def test_label_vote_device_equals_twin(n, k):
    labels = label_case(n + k, n, k)
    d = dev(labels)
    for weights, ignore in ((None, -100), (weights_for(k, n), -100), (weights_for(k, n + 1), 3)):
        got = EN.label_vote(d, weights, ignore)
        want = EN.label_vote_numpy(labels, weights, ignore)
        assert got.is_cuda and got.cpu().numpy().dtype == want.dtype and np.array_equal(got.cpu().numpy(), want)
        assert torch.equal(EN.label_vote(d, weights, ignore), got)


def test_label_vote_device_above_the_grid_cap():
    s = _csrc()
    assert re.search(r'grid_for\(n, kEnBlock, kEnLabelBlocks\)', s)
    cap = _const(s, 'kEnBlock') * _const(s, 'kEnLabelBlocks')
    n = cap + 77                                                    # a second trip through the stride loop
    labels = label_case(7, n, 2)
    got = EN.label_vote(dev(labels), [2, 1])
    assert np.array_equal(got.cpu().numpy(), EN.label_vote_numpy(labels, [2, 1]))


def test_label_vote_device_range():
    lib, p = L.lib(), torch.zeros(64, dtype=torch.int64, device='cuda').data_ptr()
    assert lib.sg_label_vote(p, 0, 4, p, -100, p, L.stream()) == -4
    assert lib.sg_label_vote(p, 33, 4, p, -100, p, L.stream()) == -4
    assert lib.sg_label_vote(p, 1, 2**31, p, -100, p, L.stream()) == -4
    assert lib.sg_label_vote(p, 2, 4, p, -100, p + 8, L.stream()) == -1          # out inside labels


# ---- links ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,k,g_total', SIZE_GRID)
def test_group_links_device_equals_twin(n, k, g_total):
    dense, labels, group = stack_case(n + g_total, n, k, g_total)
    rows = pack(dense, n, garbage=True)
    d = words(rows, n)
    for thr, measure, min_shared in ((0.5, 'iou', 1), (0.3, 'min', 1), (0.5, 'iou', 3)):
        adj = EN.mask_group_links(d, n, labels, group, thr, measure, min_shared)
        want = EN.mask_group_links_numpy(rows, n, labels, group, thr, measure, min_shared)
        assert adj.dtype == torch.int32 and host_u32(adj).shape == want.shape and np.array_equal(host_u32(adj), want)
        assert torch.equal(EN.mask_group_links(d, n, labels, group, thr, measure, min_shared), adj)
    # the components of that adjacency, on the device and on the host
    comp = ST.stitch_components(adj, g_total)
    assert comp.cpu().numpy().tolist() == ST.stitch_components_numpy(want, g_total).tolist()


def test_group_links_device_above_the_grid_cap():
    s = _csrc()
    assert re.search(r'cross_links_launch\(a, kEnLinkBlocks,', s)
    cap = _const(s, 'kEnLinkBlocks')
    g_total = 4 * (int(np.sqrt(cap)) + 2) + 1                       # tile pairs = ceil(G / 4) ** 2 > cap
    assert ((g_total + 3) // 4) ** 2 > cap and g_total <= EN.MAX_INSTANCES
    dense, labels, group = stack_case(3, 32, 8, g_total)
    rows = pack(dense, 32)
    adj = EN.mask_group_links(words(rows, 32), 32, labels, group)
    assert np.array_equal(host_u32(adj), EN.mask_group_links_numpy(rows, 32, labels, group))


def test_group_links_device_range():
    lib, p = L.lib(), torch.zeros(64, dtype=torch.int32, device='cuda').data_ptr()
    assert lib.sg_mask_group_links(p, 16385, 32, p, p, 0.5, 0, 1, p, L.stream()) == -4
    assert lib.sg_mask_group_links(p, 4, 2**31, p, p, 0.5, 0, 1, p, L.stream()) == -4
    assert lib.sg_mask_group_links(p, 4, 32, p, p, 0.5, 2, 1, p, L.stream()) == -1
    assert lib.sg_mask_group_links(p, 4, 32, p, p, float('nan'), 0, 1, p, L.stream()) == -1
    assert lib.sg_mask_group_links(p, 4, 32, p, None, 0.5, 0, 1, p, L.stream()) == -1


# ---- mask vote --------------------------------------------------------------------------------------------------------
def _vote_both(dense, n, labels, group, weights, seed):
    rows = pack(dense, n, garbage=True)
    edges = edges_of(EN.mask_group_links_numpy(rows, n, labels, group), len(dense))
    objects, obj_of, need = vote_inputs(dense, labels, group, weights, seed, edges)
    want_rows, want_np = EN.mask_vote_numpy(rows, n, obj_of, group, weights, need)
    d = words(rows, n)
    lists = EN.member_lists(objects, group, weights)
    out, npoint = EN.mask_vote(d, n, *lists, need)
    assert out.dtype == torch.int32 and npoint.cpu().numpy().dtype == want_np.dtype
    assert host_u32(out).shape == want_rows.shape and np.array_equal(host_u32(out), want_rows)
    assert np.array_equal(npoint.cpu().numpy(), want_np)
    again = EN.mask_vote(d, n, *lists, need)
    assert torch.equal(again[0], out) and torch.equal(again[1], npoint)
    return objects, obj_of, need, want_rows


@pytest.mark.parametrize('n,k,g_total', SIZE_GRID)
def test_mask_vote_device_equals_twin(n, k, g_total):
    dense, labels, group = stack_case(n + g_total, n, k, g_total)
    _vote_both(dense, n, labels, group, weights_for(k, g_total), n)


@pytest.mark.parametrize('weights', WEIGHT_SETS, ids=lambda w: f'W{sum(w)}k{len(w)}')
def test_mask_vote_device_weight_edges(weights):
    k = len(weights)
    dense, labels, group = stack_case(sum(weights) % 1000 + k, 65, k, 3 * k + 2)
    objects, obj_of, need, rows = _vote_both(dense, 65, labels, group, weights, k)
    assert np.array_equal(unpack(rows, 65), brute_mask_vote(dense, obj_of, group, weights, need))


def test_mask_vote_device_object_with_32_members():
    dense, labels, group = thirty_two_members_case()
    objects = _vote_both(dense, 2049, labels, group, [1, 2, 3, 4, 5, 6, 7, 8], 1)[0]
    assert len(objects) == 1 and len(objects[0]) == 32


def test_mask_vote_device_above_the_grid_cap():
    s = _csrc()
    assert re.search(r'grid_for\(static_cast<int64_t>\(n_obj\) \* a\.chunks, 1, kEnMaskBlocks\)', s)
    n_obj = _const(s, 'kEnMaskBlocks') + 5                          # objects x 1 chunk of words > the cap
    assert n_obj <= EN.MAX_INSTANCES
    rng = np.random.default_rng(9)
    dense = rng.random((n_obj, 32)) < 0.5
    group = np.sort(rng.integers(0, 3, n_obj)).astype(np.int32)
    objects = [[g] for g in range(n_obj)]
    rows = pack(dense, 32)
    out, npoint = EN.mask_vote(words(rows, 32), 32, *EN.member_lists(objects, group, [1, 2, 3]), np.ones(n_obj, np.int64))
    want = EN.mask_vote_numpy(rows, 32, np.arange(n_obj), group, [1, 2, 3], np.ones(n_obj, np.int64))
    assert np.array_equal(host_u32(out), want[0]) and np.array_equal(npoint.cpu().numpy(), want[1])


def test_mask_vote_device_ignores_entries_outside_their_range():
    """include/softgroup_hip.h: an entry whose row, pass or weight is outside its range is IGNORED, offsets are
    clamped into [0, n_total] -- no error status, never a wild read"""
    dense, labels, group = thirty_two_members_case(n=333)
    weights = np.array([1, 2, 3, 4, 5, 6, 7, 8])
    rows = pack(dense, 333, garbage=True)
    d = words(rows, 333)
    members = np.arange(32, dtype=np.int32)
    passes, weight = group.copy(), weights[group].astype(np.int32)
    need = np.array([18], np.int64)
    bad = {1: ('members', -5), 6: ('members', 32), 9: ('members', 2**31 - 1), 12: ('passes', -1), 13: ('passes', 32),
           20: ('weight', 0), 21: ('weight', 32768), 27: ('passes', 2**30)}
    arrays = dict(members=members.copy(), passes=passes.copy(), weight=weight.copy())
    for m, (name, value) in bad.items():
        arrays[name][m] = value
    out, npoint = EN.mask_vote(d, 333, [0, 32], arrays['members'], arrays['weight'], arrays['passes'], need)
    obj_of = np.zeros(32, np.int64)
    obj_of[list(bad)] = -1
    want = EN.mask_vote_numpy(rows, 333, obj_of, group, weights, need)
    assert np.array_equal(host_u32(out), want[0]) and np.array_equal(npoint.cpu().numpy(), want[1])
    # offsets beyond the lists, descending or negative: clamped, the object is what is left
    out, npoint = EN.mask_vote(d, 333, [0, 2**31 - 1], members, weight, passes, need)
    want = EN.mask_vote_numpy(rows, 333, np.zeros(32, np.int64), group, weights, need)
    assert np.array_equal(host_u32(out), want[0]) and np.array_equal(npoint.cpu().numpy(), want[1])
    out, npoint = EN.mask_vote(d, 333, [-7, 16, 4], members, weight, passes, [1, 1])
    want = EN.mask_vote_numpy(rows, 333, np.where(np.arange(32) < 16, 0, -1), group, weights, [1, 1])
    assert np.array_equal(host_u32(out), want[0]) and npoint.cpu().numpy().tolist() == [int(want[1][0]), 0]
    # a need outside 1 .. 32767: an empty row
    out, npoint = EN.mask_vote(d, 333, [0, 32], members, weight, passes, [0])
    assert not host_u32(out).any() and npoint.cpu().numpy().tolist() == [0]
    lib, p = L.lib(), d.data_ptr()
    assert lib.sg_mask_vote(p, 16385, 32, p, p, p, p, p, 1, p, p, L.stream()) == -4
    assert lib.sg_mask_vote(p, 4, 2**31, p, p, p, p, p, 1, p, p, L.stream()) == -4
    assert lib.sg_mask_vote(p, 4, 32, p, p, p, p, p, 16385, p, p, L.stream()) == -4
    assert lib.sg_mask_vote(p, 4, 32, p, p, p, p, p, 1, p, None, L.stream()) == -1


# ---- ensemble_results -------------------------------------------------------------------------------------------------
def same_results(got, want):
    assert got.keys() == want.keys()
    assert np.array_equal(np.asarray(got['semantic_preds']), np.asarray(want['semantic_preds']))
    assert got['semantic_preds'].dtype == want['semantic_preds'].dtype
    if 'pred_instances' in want:
        assert len(got['pred_instances']) == len(want['pred_instances'])
        for a, b in zip(got['pred_instances'], want['pred_instances']):
            assert a.keys() == b.keys()
            for key in a:
                if key == 'pred_mask' and not isinstance(b[key], dict):
                    assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key])
                else:
                    assert type(a[key]) is type(b[key]) and a[key] == b[key], key


@pytest.mark.parametrize('name', E2E_CASES)
def test_ensemble_results_device_equals_numpy(name):
    results, kw = e2e_case(name)
    got = ensemble_results(results, backend='device', **kw)
    check_e2e(got, results, kw)
    same_results(got, ensemble_results(results, backend='numpy', **kw))
    same_results(ensemble_results(results, backend='device', **kw), got)
    assert isinstance(got['semantic_preds'], np.ndarray)            # numpy in gives numpy out


def _perturbed_passes():
    """about 20 k points of scene_s2, its 12 objects as the instance list, 3 passes: as it is; one instance dropped
    and every mask eroded by a point stride; one instance duplicated and one mask cut in two"""
    xyz, _, inst = synthetic.scene_s2(seed=4, n=20000, room_scale=0.4)
    n = xyz.shape[0]
    base = [(inst == i) for i in range(12)]
    sem = np.where(inst >= 0, 2 + inst % 18, 0).astype(np.int64)
    rng = np.random.default_rng(4)

    def result(masks, flip):
        s = sem.copy()
        s[rng.random(n) < flip] = 1
        return dict(scan_id='synthetic', semantic_preds=s, coords_float=xyz,
                    pred_instances=[dict(scan_id='synthetic', label_id=int(2 + i % 18), conf=0.5 + 0.03 * i + 0.01 * j,
                                         pred_mask=rle_encode(m.astype(np.uint8))) for j, (i, m) in enumerate(masks)])

    first = [(i, m) for i, m in enumerate(base)]
    second = [(i, m & (np.arange(n) % 5 != 0)) for i, m in enumerate(base) if i != 3]
    third = first + [(7, base[7] & (np.arange(n) % 2 == 0))]
    third[2] = (2, base[2] & (np.cumsum(base[2]) <= base[2].sum() // 2))
    third.append((2, base[2] & (np.cumsum(base[2]) > base[2].sum() // 2)))
    return [result(first, 0.0), result(second, 0.2), result(third, 0.2)]


def test_ensemble_results_device_on_a_synthetic_scene():
    results = _perturbed_passes()
    for kw in ({}, dict(weights=[2, 1, 1], mask='union', thr=0.3, min_votes=1), dict(mask='all', measure='min')):
        want = ensemble_results(results, backend='numpy', **kw)
        same_results(ensemble_results(results, backend='device', **kw), want)
        assert len(want['pred_instances']) >= 11
    d_results = [dict(r, semantic_preds=torch.from_numpy(r['semantic_preds']).cuda().int()) for r in results]
    got = ensemble_results(d_results, backend='device')
    assert got['semantic_preds'].is_cuda and got['semantic_preds'].dtype == torch.int32          # CUDA stays CUDA
    assert np.array_equal(got['semantic_preds'].cpu().numpy(), want['semantic_preds'])        # (the last kw: unit weights)
    host = ensemble_results(d_results, backend='numpy')
    assert host['semantic_preds'].is_cuda and torch.equal(host['semantic_preds'], got['semantic_preds'])


def test_ensemble_results_device_range(monkeypatch):
    def one(x):
        return dict(scan_id='s', label_id=1, conf=0.5, pred_mask=dict(length=32, counts=f'{x % 32 + 1} 1'))

    results = [dict(pred_instances=[one(x) for x in range(16384)]), dict(pred_instances=[one(5)])]      # G = 16385
    with pytest.raises(L.SoftGroupHipError, match='16385'):
        ensemble_results(results, min_votes=2, backend='device')
    monkeypatch.setitem(EN._AUTO, 'instances', 'device')            # whatever 'auto' means: beyond the range, numpy
    monkeypatch.setitem(EN._AUTO, 'labels', 'device')
    got = ensemble_results(results, min_votes=2, backend='auto')['pred_instances']
    assert len(got) == 1 and got[0]['pred_mask'] == dict(length=32, counts='6 1') and got[0]['conf'] == 0.5
    # RLE runs that are not ascending
    odd = [dict(semantic_preds=np.zeros(8, np.int64),
                pred_instances=[dict(scan_id='s', label_id=1, conf=0.5, pred_mask=dict(length=8, counts='7 2 1 2'))])]
    want = ensemble_results(odd, backend='numpy')
    assert want['pred_instances'][0]['pred_mask']['counts'] == '1 2 7 2'
    with pytest.raises(ValueError):
        ensemble_results(odd, backend='device')
    same_results(ensemble_results(odd, backend='auto'), want)
