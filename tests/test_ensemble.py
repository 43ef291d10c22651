"""Several results over one cloud combined into one: the numpy twins of ``softgroup_amd.ops.ensemble`` against
plain-loop dense brute forces written here, a hand-made case for every rule, ``ensemble_results`` end to end and the
test-time-augmentation helper.  tests/test_ensemble_gpu.py runs the device on the same cases."""
import copy

import numpy as np
import pytest

from softgroup_amd.data import apply_tta, tta_scan, tta_transforms
from softgroup_amd.ops import ensemble as EN
from softgroup_amd.ops import stitch as ST
from softgroup_amd.util import ensemble_results, rle_decode, rle_encode


# ---- brute forces (plain loops over dense masks) ----------------------------------------------------------------------
def brute_label_vote(labels, weights, ignore=-100):
    labels = np.asarray(labels)
    k, n = labels.shape
    out = np.empty(n, np.int64)
    for x in range(n):
        count = {}
        for p in range(k):
            c = int(labels[p, x])
            if c >= 0 and c != ignore:
                count[c] = count.get(c, 0) + int(weights[p])
        out[x] = min(count, key=lambda c: (-count[c], c)) if count else labels[0, x]
    return out


def brute_links(dense, labels, group, thr=0.5, measure='iou', min_shared=1):
    """the edges (g, h), g < h, by the rule spelled out: python integers and one float division"""
    edges = []
    for g in range(len(dense)):
        for h in range(g + 1, len(dense)):
            if group[g] == group[h] or labels[g] != labels[h]:
                continue
            inter = int((dense[g] & dense[h]).sum())
            ca, cb = int(dense[g].sum()), int(dense[h].sum())
            den = ca + cb - inter if measure == 'iou' else min(ca, cb)
            if den > 0 and inter >= min_shared and float(inter) / float(den) > thr:
                edges.append((g, h))
    return edges


def brute_components(n, edges):
    comp = list(range(n))
    changed = True
    while changed:
        changed = False
        for g, h in edges:
            low = min(comp[g], comp[h])
            if comp[g] != low or comp[h] != low:
                comp[g] = comp[h] = low
                changed = True
    return comp


def brute_mask_vote(dense, obj_of, group, weights, need):
    n_obj, n = len(need), dense.shape[1]
    out = np.zeros((n_obj, n), bool)
    for o in range(n_obj):
        members = [g for g in range(len(dense)) if obj_of[g] == o]
        for x in range(n):
            passes = {int(group[g]) for g in members if dense[g, x]}
            out[o, x] = sum(int(weights[p]) for p in passes) >= need[o]
    return out


def pack(dense, n_bits, garbage=False):
    """uint8 rows [G, 4 * ceil(n_bits / 32)]; ``garbage`` sets every bit at and beyond n_bits in the odd rows"""
    dense = np.asarray(dense, bool).reshape(len(dense), n_bits)
    width = (n_bits + 31) // 32 * 32
    full = np.zeros((len(dense), width), bool)
    full[:, :n_bits] = dense
    if garbage:
        full[1::2, n_bits:] = True
    return np.packbits(full, axis=1, bitorder='little') if width else np.zeros((len(dense), 0), np.uint8)


def unpack(rows, n_bits):
    rows = np.ascontiguousarray(rows)
    if rows.shape[0] == 0 or n_bits == 0:
        return np.zeros((rows.shape[0], n_bits), bool)
    return np.unpackbits(rows.view(np.uint8).reshape(rows.shape[0], -1), axis=1, bitorder='little')[:, :n_bits].astype(bool)


def edges_of(adj, n):
    d = unpack(adj, n)
    assert np.array_equal(d, d.T) and not d.diagonal().any()
    return [(int(g), int(h)) for g, h in zip(*np.nonzero(d)) if g < h]


# ---- seeded cases -----------------------------------------------------------------------------------------------------
def stack_case(seed, n, k, g_total):
    """(dense bool [G, n], labels int32 [G], group int32 [G] ascending): noisy copies of a few base masks spread over
    the passes, an all-ones row, an empty row"""
    rng = np.random.default_rng(seed)
    n_base = max(1, g_total // max(k, 1))
    base = np.zeros((n_base, n), bool)
    for b in range(n_base):
        lo = int(rng.integers(0, n))
        base[b, lo:lo + max(1, int(rng.integers(1, max(2, n // 2))))] = True
    group = np.sort(rng.integers(0, k, g_total)).astype(np.int32)
    which = rng.integers(0, n_base, g_total)
    dense = base[which] ^ (rng.random((g_total, n)) < 0.08) if g_total else np.zeros((0, n), bool)
    labels = (which % 2 + 1).astype(np.int32)
    if g_total > 2:
        dense[g_total // 2] = True
        dense[g_total - 1] = False
    return dense, labels, group


def vote_inputs(dense, labels, group, weights, seed, edges=None):
    """objects of the brute links (or of ``edges``), every support kept, need drawn from {1, s // 2 + 1, s, random}"""
    rng = np.random.default_rng(seed)
    comp = brute_components(len(dense), brute_links(dense, labels, group) if edges is None else edges)
    objects, support = EN.objects_of_components(comp, group, weights)
    obj_of = np.full(len(dense), -1, np.int64)
    for o, m in enumerate(objects):
        obj_of[m] = o
    need = np.array([(1, s // 2 + 1, s, int(rng.integers(1, s + 1)))[o % 4] for o, s in enumerate(support.tolist())],
                    dtype=np.int64).reshape(-1)
    if len(objects) > 3:                                            # one instance in no object
        drop = objects.pop()
        obj_of[drop] = -1
        need = need[:-1]
    return objects, obj_of, need


# (n, K, G) -- word and wave edges x pass counts x the tile edges of the link kernel; every listed value appears
SIZE_GRID = [(1, 1, 1), (31, 2, 33), (32, 3, 33), (33, 8, 129), (63, 32, 300), (65, 2, 0), (2049, 8, 129),
             (2049, 3, 1), (70001, 3, 300), (70001, 32, 33), (33, 1, 33)]
# W = 1, 2^k - 1, 2^k, 32767: the edges of the bit planes of the device counters
WEIGHT_SETS = [[1], [1, 2, 4], [2, 2, 4], [127, 128], [128, 128], [16383, 16384], [16384, 16383], [32767],
               [1] * 31 + [32736], [1] * 32, [1000, 2000, 3000, 4000, 5000, 6000, 7000, 4767]]


def weights_for(k, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(1, 32767 // k + 1, k).astype(np.int64)


def label_case(seed, n, k):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, 5, (k, n)).astype(np.int64)
    labels[rng.random((k, n)) < 0.2] = -100
    labels[rng.random((k, n)) < 0.05] = -1
    labels[rng.random((k, n)) < 0.02] = 2**40 + 7                   # no class cap
    if n > 3:
        labels[:, 3] = -100                                         # nothing counted: pass 0's value stays
    return labels


def thirty_two_members_case(n=2049):
    """32 instances of 8 passes (4 per pass) around one base mask: one object with 32 members"""
    rng = np.random.default_rng(32)
    base = np.zeros(n, bool)
    base[100:1500] = True
    dense = base[None, :] ^ (rng.random((32, n)) < 0.02)
    return dense, np.ones(32, np.int32), np.repeat(np.arange(8), 4).astype(np.int32)


# ---- label vote -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,k', [(1, 1), (33, 2), (257, 3), (300, 8), (129, 32)])
def test_label_vote_equals_plain_loop(n, k):
    labels = label_case(n + k, n, k)
    for weights in (np.ones(k, np.int64), weights_for(k, n)):
        got = EN.label_vote_numpy(labels, weights)
        assert got.dtype == np.int64 and np.array_equal(got, brute_label_vote(labels, weights))
    assert np.array_equal(EN.label_vote_numpy(labels, None, ignore_label=3), brute_label_vote(labels, [1] * k, 3))


def test_label_vote_rules():
    ig = -100
    labels = np.array([[5, 2, ig, ig, 4, 7],
                       [3, 2, -1, ig, 9, 7],
                       [3, 9, 6, ig, 9, 8],
                       [5, 9, ig, -7, 4, 8]], dtype=np.int64)
    # a tie goes to the lowest class; ignored and negative labels are not counted; nothing counted keeps pass 0
    assert EN.label_vote_numpy(labels).tolist() == [3, 2, 6, ig, 4, 7]
    assert EN.label_vote_numpy(labels, [1, 1, 1, 2]).tolist() == [5, 9, 6, ig, 4, 8]          # weights flip winners
    assert EN.label_vote_numpy(labels[1:2]).tolist() == [3, 2, -1, ig, 9, 7]                   # K = 1
    many = np.tile(np.array([[4], [1]], np.int64), (16, 3))                                    # K = 32: 16 against 16
    assert EN.label_vote_numpy(many).tolist() == [1, 1, 1]
    assert EN.label_vote_numpy(many, [2] + [1] * 31).tolist() == [4, 4, 4]


# ---- links ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,k,g_total', [s for s in SIZE_GRID if s[0] <= 2049])
def test_group_links_equal_plain_loop(n, k, g_total):
    dense, labels, group = stack_case(n + g_total, n, k, g_total)
    rows = pack(dense, n, garbage=True)
    for thr, measure, min_shared in ((0.5, 'iou', 1), (0.3, 'min', 1), (0.5, 'iou', 3)):
        adj = EN.mask_group_links_numpy(rows, n, labels, group, thr, measure, min_shared)
        assert adj.dtype == np.uint32 and adj.shape == (g_total, (g_total + 31) // 32)
        assert edges_of(adj, g_total) == brute_links(dense, labels, group, thr, measure, min_shared)


def _bits(*sets, n=8):
    d = np.zeros((len(sets), n), bool)
    for r, s in enumerate(sets):
        d[r, list(s)] = True
    return d


def test_group_link_rules():
    # 2 of 4 points: exactly thr = 0.5 under 'iou' is NOT a link; 3 of 4 is
    d = _bits({0, 1, 2}, {1, 2, 3}, {0, 1, 2, 3})
    links = lambda *a, **kw: edges_of(EN.mask_group_links_numpy(pack(d, 8), 8, *a, **kw), len(d))      # noqa: E731
    assert links([1, 1, 1], [0, 1, 2]) == [(0, 2), (1, 2)]
    assert links([1, 1, 1], [0, 1, 1]) == [(0, 2)]                  # the same pass is never linked
    assert links([1, 1, 1], [0, 0, 0]) == []
    assert links([1, 1, 2], [0, 1, 2]) == []                        # nor a different label
    assert links([1, 1, 1], [0, 1, 2], min_shared=4) == []          # min_shared
    assert links([1, 1, 1], [0, 1, 2], min_shared=3) == [(0, 2), (1, 2)]
    assert links([1, 1, 1], [0, 1, 2], measure='min') == [(0, 1), (0, 2), (1, 2)]      # 2 / 3, 3 / 3, 3 / 3
    assert links([1, 1, 1], [0, 1, 2], thr=0.49) == [(0, 1), (0, 2), (1, 2)]
    # the decision is the one of ops.stitch.link_rule
    assert bool(ST.link_rule(2, 3, 3, 0.5, 'iou', 1)) is False and bool(ST.link_rule(2, 3, 3, 0.5, 'min', 1)) is True


# ---- objects ----------------------------------------------------------------------------------------------------------
def test_objects_chain_and_support():
    # a transitive chain across three passes: 0 - 1 - 2 (0 and 2 do not overlap enough), and a loner
    d = _bits({0, 1, 2, 3}, {2, 3, 4, 5}, {4, 5, 6, 7}, {9}, n=12)
    labels, group = [1, 1, 1, 1], [0, 1, 2, 2]
    adj = EN.mask_group_links_numpy(pack(d, 12), 12, labels, group, 0.3)
    assert edges_of(adj, 4) == [(0, 1), (1, 2)]
    comp = ST.stitch_components_numpy(adj, 4)
    objects, support = EN.objects_of_components(comp, group, [1, 2, 4])
    assert objects == [[0, 1, 2], [3]] and support.tolist() == [7, 4]
    # two members of one pass in one object count once in s
    objects, support = EN.objects_of_components([0, 0, 0, 3], [0, 1, 1, 1], [3, 5])
    assert objects == [[0, 1, 2], [3]] and support.tolist() == [8, 5]
    off, members, weight, passes = EN.member_lists([[0, 3], [1, 2]], [1, 0, 0, 0], [3, 5])
    assert off.tolist() == [0, 2, 4] and members.tolist() == [3, 0, 1, 2]          # sorted by (pass, instance)
    assert weight.tolist() == [3, 5, 3, 3] and passes.tolist() == [0, 1, 0, 0]


# ---- mask vote --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,k,g_total', [s for s in SIZE_GRID if s[0] <= 2049])
def test_mask_vote_equals_plain_loop(n, k, g_total):
    dense, labels, group = stack_case(n + g_total, n, k, g_total)
    weights = weights_for(k, g_total)
    objects, obj_of, need = vote_inputs(dense, labels, group, weights, n)
    rows, npoint = EN.mask_vote_numpy(pack(dense, n, garbage=True), n, obj_of, group, weights, need)
    assert rows.dtype == np.uint32 and rows.shape == (len(need), (n + 31) // 32) and npoint.dtype == np.int32
    want = brute_mask_vote(dense, obj_of, group, weights, need)
    assert np.array_equal(unpack(rows, n), want) and npoint.tolist() == want.sum(1).tolist()
    assert rows.tobytes() == pack(want, n).tobytes()                # bits beyond n_bits are 0


def test_mask_vote_rules():
    # two members of pass 0 hold point 1: the pass counts once there
    d = _bits({0, 1}, {1, 2}, {1, 2, 3}, {0, 1, 2, 3})
    group, obj_of = [0, 0, 1, 2], [0, 0, 0, 0]
    vote = lambda w, need: unpack(EN.mask_vote_numpy(pack(d, 8), 8, obj_of, group, w, [need])[0], 8)[0].nonzero()[0].tolist()      # noqa: E731
    assert vote([1, 1, 1], 3) == [1, 2]                             # 'all'
    assert vote([1, 1, 1], 2) == [0, 1, 2, 3]                       # 'majority' of s = 3
    assert vote([1, 1, 1], 1) == [0, 1, 2, 3]                       # 'union'
    assert vote([5, 1, 1], 6) == [0, 1, 2]                          # not 5 + 5 at point 1, and 2 at point 3
    # exactly half is out under 'majority': s = 4, need 3
    d2 = _bits({0, 1, 2}, {0, 1, 2}, {0, 1}, {0})
    got = EN.mask_vote_numpy(pack(d2, 8), 8, [0, 0, 0, 0], [0, 1, 2, 3], [1, 1, 1, 1], [4 // 2 + 1])
    assert unpack(got[0], 8)[0].nonzero()[0].tolist() == [0, 1] and got[1].tolist() == [2]
    # W = 32767
    got = EN.mask_vote_numpy(pack(d2[:2], 8), 8, [0, 0], [0, 1], [32766, 1], [32767])
    assert got[1].tolist() == [3]
    got = EN.mask_vote_numpy(pack(d2[1:3], 8), 8, [0, 0], [0, 1], [32766, 1], [32767])
    assert unpack(got[0], 8)[0].nonzero()[0].tolist() == [0, 1]
    with pytest.raises(ValueError):
        EN.mask_vote_numpy(pack(d2, 8), 8, [0, 0, 0, 0], [0, 1, 2, 3], [1, 1, 1, 1], [0])
    # an instance in no object takes no part
    got = EN.mask_vote_numpy(pack(d2, 8), 8, [0, -1, -1, 0], [0, 1, 2, 3], [1, 1, 1, 1], [1])
    assert unpack(got[0], 8)[0].nonzero()[0].tolist() == [0, 1, 2]


@pytest.mark.parametrize('weights', WEIGHT_SETS, ids=lambda w: f'W{sum(w)}k{len(w)}')
def test_mask_vote_weight_edges(weights):
    k = len(weights)
    dense, labels, group = stack_case(sum(weights) % 1000 + k, 65, k, 3 * k + 2)
    objects, obj_of, need = vote_inputs(dense, labels, group, weights, k)
    rows, npoint = EN.mask_vote_numpy(pack(dense, 65), 65, obj_of, group, weights, need)
    want = brute_mask_vote(dense, obj_of, group, weights, need)
    assert np.array_equal(unpack(rows, 65), want) and npoint.tolist() == want.sum(1).tolist()


def test_pass_weights():
    assert EN.pass_weights(None, 3).tolist() == [1, 1, 1]
    assert EN.pass_weights([2.0, np.int32(3)], 2).tolist() == [2, 3]
    assert EN.pass_weights([32767], 1).tolist() == [32767]
    for bad, k in (([1.5, 1], 2), ([0, 1], 2), ([1, -1], 2), ([1], 2), ([32767, 1], 2), (None, 0), (None, 33),
                   ([float('nan')], 1), (['a'], 1), ([True], 1)):
        with pytest.raises(ValueError):
            EN.pass_weights(bad, k)


# ---- ensemble_results -------------------------------------------------------------------------------------------------
def _inst(n, points, label, conf, dense=False, **more):
    m = np.zeros(n, np.uint8)
    m[list(points)] = 1
    return dict(dict(scan_id='scene', label_id=label, conf=conf, pred_mask=m.astype(bool) if dense else rle_encode(m)),
                **more)


def _mask_of(inst, n):
    m = inst['pred_mask']
    return rle_decode(m).astype(bool) if isinstance(m, dict) else np.asarray(m).astype(bool)


def brute_ensemble(results, weights=None, thr=0.5, measure='iou', min_shared=1, min_votes=None, mask='majority',
                   min_npoint=0, ignore_label=-100):
    """(voted labels or None, [(first member, label, conf, dense mask)]) from the rules, dense and in plain loops"""
    k = len(results)
    w = [1] * k if weights is None else [int(x) for x in weights]
    total = sum(w)
    min_votes = total // 2 + 1 if min_votes is None else min_votes
    sem = None
    if 'semantic_preds' in results[0]:
        sem = brute_label_vote(np.stack([np.asarray(r['semantic_preds']) for r in results]), w, ignore_label)
    flat = [(p, inst) for p, r in enumerate(results) for inst in r.get('pred_instances', [])]
    if not flat:
        return sem, []
    n = len(_mask_of(flat[0][1], None))
    dense = np.stack([_mask_of(inst, n) for _, inst in flat])
    group = [p for p, _ in flat]
    labels = [inst['label_id'] for _, inst in flat]
    comp = brute_components(len(flat), brute_links(dense, labels, group, thr, measure, min_shared))
    out = []
    for root in sorted(set(comp)):
        members = [g for g in range(len(flat)) if comp[g] == root]
        passes = sorted({group[g] for g in members})
        s = sum(w[p] for p in passes)
        if s < min_votes:
            continue
        need = {'majority': s // 2 + 1, 'union': 1, 'all': s}[mask]
        v = np.zeros(n, np.int64)
        for p in passes:
            held = np.zeros(n, bool)
            for g in members:
                if group[g] == p:
                    held |= dense[g]
            v += w[p] * held
        voted = v >= need
        if voted.sum() < min_npoint:
            continue
        acc = np.float64(0.0)
        for p in passes:
            acc = acc + np.float64(w[p]) * np.float64(max(flat[g][1]['conf'] for g in members if group[g] == p))
        out.append((flat[members[0]][1], labels[members[0]], float(acc / np.float64(total)), voted))
    return sem, out


def e2e_case(name):
    """-> (results, keyword arguments)"""
    n = 97
    rng = np.random.default_rng(5)
    sem = rng.integers(0, 4, (4, n)).astype(np.int64)
    sem[1, 10:20] = -100
    a = lambda **kw: _inst(n, range(0, 40), 1, 0.9, **kw)           # noqa: E731
    if name in ('three_pass', 'weighted', 'union', 'all', 'min_votes_1', 'min_npoint', 'bool_masks'):
        d = name == 'bool_masks'
        results = [
            dict(semantic_preds=sem[0], offset_preds=np.zeros((n, 3), np.float32), scan_id='scene',
                 panoptic_preds=np.arange(n), pred_instances=[a(dense=d), _inst(n, range(50, 70), 2, 0.5, dense=d),
                                                              _inst(n, range(90, 97), 3, 0.3, dense=d)]),
            dict(semantic_preds=sem[1], offset_preds=np.ones((n, 3), np.float32), scan_id='scene',
                 panoptic_preds=np.arange(n), pred_instances=[_inst(n, range(4, 44), 1, 0.8, dense=d),
                                                              _inst(n, range(0, 12), 1, 0.95, dense=d),
                                                              _inst(n, range(52, 75), 2, 0.7, dense=d)]),
            dict(semantic_preds=sem[2], offset_preds=np.ones((n, 3), np.float32), scan_id='scene',
                 panoptic_preds=np.arange(n), pred_instances=[_inst(n, range(50, 70), 3, 0.6, dense=d),
                                                              _inst(n, range(2, 38), 1, 0.7, dense=d)]),
        ]
        kw = {'three_pass': {}, 'weighted': dict(weights=[1, 3, 1], thr=0.25), 'union': dict(mask='union', thr=0.2),
              'all': dict(mask='all', thr=0.2, measure='min'), 'min_votes_1': dict(min_votes=1),
              'min_npoint': dict(min_votes=1, min_npoint=8), 'bool_masks': dict(min_votes=1)}[name]
        return results, kw
    if name == 'k1':
        return [dict(semantic_preds=sem[0].astype(np.int32), pred_instances=[a(extra='kept'), _inst(n, [], 2, 0.1),
                                                                             _inst(n, range(3), 2, 0.2)])], \
            dict(min_npoint=1)
    if name == 'empty_lists':
        return [dict(semantic_preds=sem[p], pred_instances=[]) for p in range(3)], {}
    if name == 'one_empty_pass':
        return [dict(semantic_preds=sem[0], pred_instances=[]), dict(semantic_preds=sem[1], pred_instances=[a()]),
                dict(semantic_preds=sem[2], pred_instances=[a()]), dict(semantic_preds=sem[3], pred_instances=[a()])], \
            dict(weights=[4, 1, 2, 1])
    if name == 'no_instances_key':
        return [dict(semantic_preds=sem[p]) for p in range(2)], {}
    raise KeyError(name)


E2E_CASES = ['three_pass', 'weighted', 'union', 'all', 'min_votes_1', 'min_npoint', 'bool_masks', 'k1', 'empty_lists',
             'one_empty_pass', 'no_instances_key']


def check_e2e(out, results, kw):
    """``out`` against the brute force: labels, order, label_id, conf to the last bit, masks in the canonical form"""
    sem, want = brute_ensemble(results, **kw)
    assert np.array_equal(np.asarray(out['semantic_preds']), sem)
    assert out['semantic_preds'].dtype == results[0]['semantic_preds'].dtype
    assert 'panoptic_preds' not in out
    if 'pred_instances' not in results[0]:
        assert 'pred_instances' not in out
        return
    got = out['pred_instances']
    assert len(got) == len(want)
    for inst, (first, label, conf, voted) in zip(got, want):
        assert inst['label_id'] == label and inst['scan_id'] == first['scan_id']
        assert isinstance(inst['conf'], float) and inst['conf'] == conf
        if isinstance(first['pred_mask'], dict):
            assert inst['pred_mask'] == rle_encode(voted.astype(np.uint8))
        else:
            assert inst['pred_mask'].dtype == np.bool_ and np.array_equal(inst['pred_mask'], voted)
        assert {k: v for k, v in inst.items() if k not in ('conf', 'pred_mask')} == \
            {k: v for k, v in first.items() if k not in ('conf', 'pred_mask')}


@pytest.mark.parametrize('name', E2E_CASES)
def test_ensemble_results_equal_plain_loop(name):
    results, kw = e2e_case(name)
    before = copy.deepcopy(results)
    out = ensemble_results(results, backend='numpy', **kw)
    check_e2e(out, results, kw)
    for r, b in zip(results, before):                               # inputs not modified
        assert r.keys() == b.keys() and np.array_equal(r['semantic_preds'], b['semantic_preds'])
        assert [(i['conf'], str(i['pred_mask'])) for i in r.get('pred_instances', [])] == \
            [(i['conf'], str(i['pred_mask'])) for i in b.get('pred_instances', [])]
    for key in results[0]:
        if key not in ('semantic_preds', 'pred_instances', 'panoptic_preds'):
            assert out[key] is results[0][key]                      # copied from pass 0
    check_e2e(ensemble_results(results, backend='numpy', **kw), results, kw)


def test_ensemble_results_hand_case():
    results, _ = e2e_case('three_pass')
    out = ensemble_results(results, backend='numpy')
    got = out['pred_instances']
    # objects in the order of their smallest member: {0, 3, 7} label 1 (pass 1's second label-1 instance overlaps too
    # little), {1, 5} label 2; label 3 of pass 0 and of pass 2 do not overlap, each has support 1 < 2
    assert [i['label_id'] for i in got] == [1, 2]
    assert got[0]['conf'] == float((np.float64(0.9) + np.float64(0.8) + np.float64(0.7)) / np.float64(3))
    assert got[1]['conf'] == float((np.float64(0.5) + np.float64(0.7)) / np.float64(3))
    assert rle_decode(got[0]['pred_mask']).nonzero()[0].tolist() == list(range(2, 40))
    assert rle_decode(got[1]['pred_mask']).nonzero()[0].tolist() == list(range(52, 70))      # 2 of s = 2 needed
    assert got[0]['pred_mask']['length'] == 97
    keep_all = ensemble_results(results, min_votes=1, backend='numpy')['pred_instances']
    assert [i['label_id'] for i in keep_all] == [1, 2, 3, 1, 3]     # ascending smallest member
    assert out['offset_preds'] is results[0]['offset_preds'] and out['scan_id'] == 'scene'


def test_ensemble_results_min_votes_default_and_bounds():
    results, _ = e2e_case('three_pass')
    assert str(ensemble_results(results, backend='numpy')) == str(ensemble_results(results, min_votes=2, backend='numpy'))
    w = dict(weights=[1, 3, 1])                                     # W = 5: default 3
    assert str(ensemble_results(results, backend='numpy', **w)) == \
        str(ensemble_results(results, min_votes=3, backend='numpy', **w))
    for bad in (0, 6, 2.5, -1):
        with pytest.raises(ValueError):
            ensemble_results(results, min_votes=bad, backend='numpy', **w)
    ensemble_results(results, min_votes=5, backend='numpy', **w)


def test_ensemble_results_errors():
    results, _ = e2e_case('three_pass')
    with pytest.raises(ValueError):
        ensemble_results([], backend='numpy')                       # K = 0
    with pytest.raises(ValueError):
        ensemble_results([results[0]] * 33, backend='numpy')        # K = 33
    for weights in ([1, 1], [1, 1.5, 1], [1, 0, 1], [32767, 1, 1]):
        with pytest.raises(ValueError):
            ensemble_results(results, weights=weights, backend='numpy')
    short = dict(results[1], semantic_preds=results[1]['semantic_preds'][:-1])
    with pytest.raises(ValueError, match='semantic_preds'):
        ensemble_results([results[0], short], backend='numpy')
    other = dict(results[1], pred_instances=[_inst(96, range(5), 1, 0.5)])
    with pytest.raises(ValueError, match='pred_instances'):
        ensemble_results([results[0], other], backend='numpy')
    lacks = {k: v for k, v in results[1].items() if k != 'offset_preds'}
    with pytest.raises(ValueError, match='offset_preds'):
        ensemble_results([results[0], lacks], backend='numpy')
    with pytest.raises(ValueError, match='offset_preds'):
        ensemble_results([lacks, results[0]], backend='numpy')
    for kw in (dict(mask='most'), dict(measure='dice'), dict(min_npoint=-1), dict(backend='gpu')):
        with pytest.raises(ValueError):
            ensemble_results(results, **dict(dict(backend='numpy'), **kw))


def test_ensemble_results_tensors_and_lazy_lists():
    import torch
    results, kw = e2e_case('weighted')
    as_tensor = [dict(r, semantic_preds=torch.from_numpy(r['semantic_preds']).int()) for r in results]
    out = ensemble_results(tuple(as_tensor), backend='numpy', **kw)
    assert torch.is_tensor(out['semantic_preds']) and out['semantic_preds'].dtype == torch.int32
    want = ensemble_results(results, backend='numpy', **kw)
    assert np.array_equal(out['semantic_preds'].numpy(), want['semantic_preds'])
    assert str(out['pred_instances']) == str(want['pred_instances'])


# ---- test-time augmentation -------------------------------------------------------------------------------------------
def test_tta_transforms():
    ms = tta_transforms()
    assert len(ms) == 4 and np.array_equal(ms[0], np.eye(3)) and all(m.shape == (3, 3) for m in ms)
    assert np.array_equal(ms[1], [[0, -1, 0], [1, 0, 0], [0, 0, 1]]) and np.array_equal(ms[2], np.diag([-1, -1, 1]))
    ms = tta_transforms(rot90=(1, 0, 5), flip_x=(True, False))
    assert np.array_equal(ms[0], np.eye(3)) and len(ms) == 4        # the identity first, every matrix once
    assert np.array_equal(ms[2], np.diag([-1.0, 1.0, 1.0]))
    for m in tta_transforms((0, 1, 2, 3), (False, True)):
        assert np.array_equal(np.abs(m).sum(0), [1, 1, 1]) and np.array_equal(np.abs(m).sum(1), [1, 1, 1])
    assert len(tta_transforms((0, 1, 2, 3), (False, True))) == 8


def test_apply_tta_signed_permutations_are_exact():
    rng = np.random.default_rng(0)
    xyz = (rng.standard_normal((1000, 3)) * 1e3).astype(np.float32)
    xyz[0] = [0.0, -0.0, np.float32(1e-40)]
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    want = {0: (x, y, z), 1: (-y, x, z), 2: (-x, -y, z), 3: (y, -x, z)}
    for r, m in enumerate(tta_transforms()):
        got = apply_tta(xyz, m)
        assert got.dtype == np.float32 and got is not xyz
        assert np.array_equal(got.view(np.uint32), np.stack(want[r], 1).view(np.uint32))      # bit for bit
    got = apply_tta(xyz, tta_transforms((1, ), (True, ))[1])        # mirror, then a quarter turn: (-x, y) -> (-y, -x)
    assert np.array_equal(got.view(np.uint32), np.stack([-y, -x, z], 1).view(np.uint32))
    import torch
    t = apply_tta(torch.from_numpy(xyz), tta_transforms()[3])
    assert np.array_equal(t.numpy().view(np.uint32), np.stack(want[3], 1).view(np.uint32))
    # any other matrix: float64, one cast
    th = 0.35 * np.pi
    m = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    assert np.array_equal(apply_tta(xyz, m), (xyz.astype(np.float64) @ m.T).astype(np.float32))
    with pytest.raises(ValueError):
        apply_tta(xyz, np.eye(2))


def test_tta_scan_with_a_fake_run():
    results, kw = e2e_case('three_pass')
    xyz = np.arange(97 * 3, dtype=np.float32).reshape(97, 3)
    seen = []

    def run(xyz_t, tag):
        seen.append((xyz_t.copy(), tag))
        return results[len(seen) - 1]

    out = tta_scan(run, xyz, 'feats', transforms=tta_transforms((0, 1, 2)), backend='numpy', **kw)
    assert [tag for _, tag in seen] == ['feats'] * 3 and np.array_equal(seen[0][0], xyz)
    assert np.array_equal(seen[1][0], np.stack([-xyz[:, 1], xyz[:, 0], xyz[:, 2]], 1))
    assert str(out) == str(ensemble_results(results, backend='numpy', **kw))
