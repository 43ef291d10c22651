"""Greedy mask NMS (softgroup_amd.ops.mask_nms / util.nms_instances / test_cfg.nms) on the host.

The yardstick is ``brute`` below: dense bool masks, the rules of include/softgroup_hip.h taken literally
(descending score, lower index first among equals; a kept mask suppresses the later, not yet suppressed masks of
its class with inter / den > thr in one double division; den == 0 suppresses nothing; a suppressed mask
suppresses nobody).  It is not the package's numpy backend.  Everything is compared for equality.
The reference has no NMS step, so there is no reference output to compare with."""
import functools

import numpy as np
import pytest
import torch

from softgroup_amd import ops, synthetic
from softgroup_amd.ops import nms as MN
from softgroup_amd.util import nms_instances, rle_decode, rle_encode

MODES = [(ag, me) for ag in (False, True) for me in ('iou', 'min')]
SHAPES = [(67, 2049), (130, 70001), (300, 4097), (2900, 64)]
SMALL = [(1, 1), (7, 31), (9, 33)]
THR = 0.5


def gen(seed, n, N, classes=3, nscore=8):
    G = max(2, n // 3)
    r = np.random.default_rng(seed)
    base = np.zeros((G, N), bool)
    for g in range(G):
        c = r.integers(0, N)
        w = max(1, int(N * r.uniform(0.03, 0.15)))
        base[g, (c + np.arange(w)) % N] = r.random(w) < 0.8
    which = r.integers(0, G, n)
    p = r.uniform(0.05, 0.5, n)
    m = base[which] & (r.random((n, N)) >= p[:, None])
    m |= r.random((n, N)) < 0.002
    if n > 3:
        m[r.integers(0, n)] = False            # one empty mask
    return m, (r.integers(0, nscore, n) / nscore).astype(np.float32), r.integers(0, classes, n).astype(np.int32)


def brute(m, scores, labels, thr, measure, class_agnostic, inter=None):
    """-> (keep uint8 [n], inter int32 [n, n]); the inner loop over the later masks is written with arrays"""
    m = np.asarray(m, bool)
    n = m.shape[0]
    if inter is None:
        inter = m.astype(np.int32) @ m.T
    cnt = inter.diagonal().astype(np.int64)
    order = sorted(range(n), key=lambda i: (-float(scores[i]), i))     # (-0.0 == 0.0: the index decides)
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)
    suppressed = np.zeros(n, bool)
    keep = np.zeros(n, np.uint8)
    for i in order:
        if suppressed[i]:
            continue
        keep[i] = 1
        cand = (pos > pos[i]) & ~suppressed
        if not class_agnostic and labels is not None:
            cand &= labels == labels[i]
        it = inter[i].astype(np.int64)
        den = cnt[i] + cnt - it if measure == 'iou' else np.minimum(cnt[i], cnt)
        cand &= den != 0
        j = np.flatnonzero(cand)
        suppressed[j[it[j].astype(np.float64) / den[j].astype(np.float64) > thr]] = True
    return keep, inter


@functools.lru_cache(maxsize=None)
def case(n, N, seed=0):
    """(masks, scores, labels, inter) of one generated case, computed once and shared (read only)"""
    m, s, lab = gen(seed, n, N)
    inter = m.astype(np.int32) @ m.T
    for a in (m, s, lab, inter):
        a.setflags(write=False)
    return m, s, lab, inter


def reference(n, N, measure, class_agnostic, seed=0):
    m, s, lab, inter = case(n, N, seed)
    keep, _ = brute(m, s, lab, THR, measure, class_agnostic, inter)
    return m, s, lab, inter, keep


def bits_of(m):
    """dense [n, N] -> int32 bit rows [n, ceil(N / 32)]"""
    n, N = m.shape
    return MN.pack_masks(m, N).view(np.int32).reshape(n, (N + 31) // 32)


@pytest.mark.parametrize('agnostic,measure', MODES)
@pytest.mark.parametrize('n,N', SHAPES + SMALL)
def test_numpy_backend_equals_brute_force(n, N, agnostic, measure):
    m, s, lab, inter, keep = reference(n, N, measure, agnostic)
    if (n, N) in SHAPES:
        assert 0.10 <= 1.0 - keep.mean() <= 0.95
    got, n_keep, got_inter = MN.mask_nms_numpy(MN.pack_masks(m, N), N, s, lab, THR, measure, agnostic,
                                               return_inter=True)
    assert got.dtype == np.uint8 and np.array_equal(got, keep) and n_keep == int(keep.sum())
    assert got_inter.dtype == np.int32 and np.array_equal(got_inter, inter)
    lazy, _, none = MN.mask_nms_numpy(MN.pack_masks(m, N), N, s, lab, THR, measure, agnostic)
    assert none is None and np.array_equal(lazy, keep)


def test_generated_cases_tell_the_rules_apart():
    """the cases must be able to fail an implementation that is not greedy, that breaks ties the other way, or that
    ignores the class"""
    m, s, lab, inter = case(300, 4097)
    keep, _ = brute(m, s, lab, THR, 'iou', False, inter)
    other_tie, _ = brute(m[::-1], s[::-1], lab[::-1], THR, 'iou', False, inter[::-1, ::-1])
    assert (other_tie[::-1] != keep).sum() >= 1
    agnostic, _ = brute(m, s, lab, THR, 'iou', True, inter)
    assert (agnostic != keep).sum() >= 1


def test_ops_mask_nms_cpu_tensors():
    m, s, lab, inter, keep = reference(67, 2049, 'iou', False)
    bits = bits_of(m).copy()
    bits[:, -1] |= np.int32(-1) << np.int32(2049 % 32)       # bits at and beyond N are ignored
    k, nk, it = ops.mask_nms(torch.from_numpy(bits), 2049, torch.from_numpy(s.copy()), torch.from_numpy(lab.copy()), thr=THR,
                             return_inter=True)
    assert not k.is_cuda and k.dtype == torch.uint8 and nk.dtype == torch.int32 and it.dtype == torch.int32
    assert np.array_equal(k.numpy(), keep) and int(nk) == keep.sum() and np.array_equal(it.numpy(), inter)
    k2, _ = ops.mask_nms(torch.from_numpy(bits), 2049, torch.from_numpy(s.copy()), None, thr=THR)
    assert np.array_equal(k2.numpy(), brute(m, s, None, THR, 'iou', True, inter)[0])
    with pytest.raises(ValueError):
        ops.mask_nms(torch.from_numpy(bits), 2049, torch.from_numpy(s.copy()), measure='dice')


# ---- hand-made cases (shared with the GPU tests) ----------------------------------------------------------------
def _rows(N, *point_sets):
    m = np.zeros((len(point_sets), N), bool)
    for k, pts in enumerate(point_sets):
        m[k, list(pts)] = True
    return m


HAND = {
    # A suppresses B; B alone would have suppressed C, A does not: C is kept
    'chain': (_rows(40, range(0, 20), range(8, 24), range(12, 26)), [0.9, 0.8, 0.7], [1, 1, 1], 0.35, 'iou',
              [1, 0, 1]),
    # inter 1, union 2: the quotient equals thr and is not above it
    'equal_thr': (_rows(33, [0], [0, 32]), [0.9, 0.8], [0, 0], 0.5, 'iou', [1, 1]),
    'above_thr': (_rows(33, [0], [0, 32]), [0.9, 0.8], [0, 0], 0.49, 'iou', [1, 0]),
    # all scores equal: the lower index goes first
    'all_equal': (_rows(10, range(0, 6), range(0, 7), range(0, 8)), [0.5, 0.5, 0.5], [2, 2, 2], 0.5, 'iou',
                  [1, 0, 0]),
    'zero_signs': (_rows(10, range(0, 6), range(0, 7)), [0.0, -0.0], [2, 2], 0.5, 'iou', [1, 0]),
    'zero_signs_2': (_rows(10, range(0, 6), range(0, 7)), [-0.0, 0.0], [2, 2], 0.5, 'iou', [1, 0]),
    # two empty masks: den == 0 suppresses nothing, with either measure
    'empty_iou': (_rows(12, [], [], range(3)), [0.3, 0.9, 0.5], [1, 1, 1], 0.0, 'iou', [1, 1, 1]),
    'empty_min': (_rows(12, [], [], range(3)), [0.3, 0.9, 0.5], [1, 1, 1], 0.0, 'min', [1, 1, 1]),
    # 'min': a small mask inside a large one
    'inside_min': (_rows(70, range(64), range(60, 66)), [0.9, 0.8], [1, 1], 0.6, 'min', [1, 0]),
    'inside_iou': (_rows(70, range(64), range(60, 66)), [0.9, 0.8], [1, 1], 0.6, 'iou', [1, 1]),
    # another class is left alone
    'classes': (_rows(10, range(8), range(8)), [0.9, 0.8], [1, 2], 0.5, 'iou', [1, 1]),
}


@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_made_cases(name):
    m, s, lab, thr, measure, want = HAND[name]
    s, lab = np.array(s, np.float32), np.array(lab, np.int32)
    assert brute(m, s, lab, thr, measure, False)[0].tolist() == want        # the yardstick itself
    got, n_keep, _ = MN.mask_nms_numpy(MN.pack_masks(m, m.shape[1]), m.shape[1], s, lab, thr, measure)
    assert got.tolist() == want and n_keep == sum(want)


def test_no_masks():
    keep, n_keep, inter = MN.mask_nms_numpy(np.zeros((0, 8), np.uint8), 40, np.zeros(0, np.float32), None,
                                            return_inter=True)
    assert keep.shape == (0, ) and n_keep == 0 and inter.shape == (0, 0)
    k, nk = ops.mask_nms(torch.zeros((0, 2), dtype=torch.int32), 40, torch.zeros(0))
    assert k.numel() == 0 and int(nk) == 0
    assert nms_instances([]) == []


# ---- nms_instances ------------------------------------------------------------------------------------------------
def instance_list(m, s, lab, rle):
    return [dict(scan_id='s', label_id=int(lab[k]), conf=s[k], pred_mask=rle_encode(m[k]) if rle else m[k].copy())
            for k in range(len(m))]


@pytest.mark.parametrize('rle', [True, False], ids=['rle', 'bool'])
@pytest.mark.parametrize('agnostic,measure', MODES)
def test_nms_instances_numpy(rle, agnostic, measure):
    m, s, lab, _, keep = reference(67, 2049, measure, agnostic)
    insts = instance_list(m, s, lab, rle)
    out = nms_instances(insts, THR, measure, agnostic, backend='numpy')
    want = [insts[k] for k in np.flatnonzero(keep)]
    assert len(out) == len(want) and all(a is b for a, b in zip(out, want))
    auto = nms_instances(insts, THR, measure, agnostic)
    assert [id(a) for a in auto] == [id(a) for a in want]
    with pytest.raises(ValueError):
        nms_instances(insts, backend='cuda')


# ---- SoftGroup.get_instances on CPU tensors ----------------------------------------------------------------------
def _heads(seed=0, n_pts=3000, n_groups=5, n_prop=14):
    """proposals that overlap heavily (several noisy copies of a few point sets) and random head outputs"""
    r = np.random.default_rng(seed)
    pairs = []
    for p in range(n_prop):
        c = (p % n_groups) * (n_pts // n_groups)
        pts = c + np.flatnonzero(r.random(n_pts // n_groups) < r.uniform(0.6, 0.95))
        pairs.append(np.stack([np.full(pts.size, p), pts], 1))
    pidx = torch.from_numpy(np.concatenate(pairs)).int()
    g = torch.Generator().manual_seed(seed)
    sem = torch.randn(n_pts, 20, generator=g)
    cls_s = torch.randn(n_prop, 19, generator=g) * 2
    iou_s = torch.rand(n_prop, 19, generator=g)
    mask_s = torch.randn(pidx.size(0), 19, generator=g) + 1.0
    return pidx, sem, cls_s, iou_s, mask_s


@pytest.mark.parametrize('nms', [dict(thr=0.4, measure='iou', class_agnostic=False),
                                 dict(thr=0.6, measure='min', class_agnostic=True)], ids=['iou', 'min_agnostic'])
def test_get_instances_cpu_filters_by_brute_force(nms):
    model = synthetic.build_model(seed=0, device='cpu')
    heads = _heads()
    base_cfg = dict(model.test_cfg)
    with torch.no_grad():
        plain = model.get_instances('s', *heads)
        model.test_cfg = dict(base_cfg, nms=None)
        none = model.get_instances('s', *heads)
        model.test_cfg = dict(base_cfg, nms=nms)
        got = model.get_instances('s', *heads)
    assert len(none) == len(plain) > 20
    for a, b in zip(none, plain):
        assert a['label_id'] == b['label_id'] and a['conf'] == b['conf'] and a['pred_mask'] == b['pred_mask']
    m = np.stack([rle_decode(p['pred_mask']) for p in plain]).astype(bool)
    keep, _ = brute(m, np.array([p['conf'] for p in plain], np.float32),
                    np.array([p['label_id'] for p in plain], np.int32), nms['thr'], nms['measure'],
                    nms['class_agnostic'])
    assert 0 < keep.sum() < len(plain)
    want = [plain[k] for k in np.flatnonzero(keep)]
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a['label_id'] == b['label_id'] and a['conf'] == b['conf'] and a['pred_mask'] == b['pred_mask']
