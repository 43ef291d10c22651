"""softgroup_amd.util.visualize with backend='device' (viz_io.hip, through the C ABI): the golden PLY files of the
reference (tests/golden/visualization_golden.json) with the proof, from the kernels' meta block, that the device
printed them itself -- and the opposite for the cases it must decline; the float formatter over a million
float32 bit patterns against the host's '%f'; the paint from bit rows and from runs against a dense numpy paint
at the size of a scan; the tie rule; one 150 000-point scan end to end.  Text and integers: no tolerance."""
import base64
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from softgroup_amd import _lib as L  # noqa: E402
from softgroup_amd.util import results as R  # noqa: E402
from softgroup_amd.util import visualize as V  # noqa: E402
from softgroup_amd.util.rle import rle_encode  # noqa: E402
from test_visualization import (CASES, GOLD, Dataset, check_result_equals_tree, check_task, check_ties, mg,  # noqa: E402
                                vc)

pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def declines(case, task):
    return case['declines'] == 'all' or task in case['declines']


@pytest.mark.parametrize('task', vc.TASKS)
@pytest.mark.parametrize('name', sorted(CASES))
def test_device_backend_matches_reference(name, task, tmp_path):
    case = CASES[name]
    vc.write_tree(case, str(tmp_path))
    info = check_task(case, task, str(tmp_path), 'device')
    if info is None:
        return
    print(name, task, {k: info[k] for k in ('formatted_by', 'declined', 'vertices', 'bytes')})
    if declines(case, task):
        # the kernels refuse (meta: declined rows / colour components) and numpy prints the same bytes
        assert info['declined'] != 0 and info['formatted_by'] == 'numpy'
        other, = V.save_visualizations(str(tmp_path), [case['room']], [task], str(tmp_path / 'np'), backend='numpy')
        assert open(other['path'], 'rb').read() == open(info['path'], 'rb').read()
    else:
        # no silent fall back: the device formatted every kept row
        assert info['declined'] == 0 and info['formatted_by'] == 'device'


def ply_vertices(xyz, rgb=None, keep=None, offset=None):
    """sg_viz_ply_vertices on its own -> (bytes, lines, declined, dropped)"""
    lib = L.lib()
    n = len(xyz)
    cap = 69 * n
    xd = dev(xyz, np.float32)
    cd = dev(np.zeros((n, 3), np.uint8) if rgb is None else rgb, np.uint8)
    kd = None if keep is None else dev(keep, np.uint8)
    od = None if offset is None else dev(offset, np.float32)
    text = torch.empty(max(cap, 16), dtype=torch.uint8, device='cuda')
    meta = torch.full((4, ), -1, dtype=torch.int64, device='cuda')
    ws = L.workspace(lib.sg_viz_ply_vertices_workspace_bytes(n), 'cuda')
    L.check(lib.sg_viz_ply_vertices(L.ptr(xd), L.ptr(od), L.ptr(cd), L.ptr(kd), n, L.ptr(text), cap, L.ptr(meta),
                                    L.ptr(ws), ws.numel(), L.stream()), 'sg_viz_ply_vertices')
    total, lines, declined, dropped = meta.cpu().tolist()
    return text[:total].cpu().numpy().tobytes(), lines, declined, dropped


def boundary_patterns(rng, count):
    """float32 values next to a rounding boundary (k + 1/2) * 10^-6, k log-uniform up to 2^31 * 10^6: the nearest
    float32 and its two neighbours"""
    k = np.floor(np.exp(rng.uniform(0, np.log(2.0**31 * 1e6 - 1), size=count)))
    k[:1000] = np.arange(1000)
    x = ((k + 0.5) / 1e6).astype(np.float32)
    x = np.concatenate([np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(np.inf))])
    return x * rng.choice(np.array([-1, 1], np.float32), size=x.size)


def test_float_formatter_over_a_million_bit_patterns():
    rng = np.random.default_rng(2024)
    # uniform over the accepted bit patterns: a sign and a magnitude below 2^31 (biased exponent 158)
    bits = rng.integers(0, 158 << 23, size=900000, dtype=np.uint64) | (rng.integers(0, 2, size=900000, dtype=np.uint64) << 31)
    x = np.concatenate([bits.astype(np.uint32).view(np.float32),boundary_patterns(rng, 110000), vc.formatter_values(),
                        np.array([j / 128.0 for j in range(-300, 300)], np.float32)])
    x = x[np.isfinite(x) & (np.abs(x) < 2.0**31)]
    x = x[:len(x) // 3 * 3]
    assert x.size >= 1000000
    text, lines, declined, dropped = ply_vertices(x.reshape(-1, 3))
    assert (lines, declined, dropped) == (x.size // 3, 0, 0)
    got = text.decode().split('\n')
    want = ['%f %f %f 0 0 0' % (a, b, c) for a, b, c in x.astype(np.float64).reshape(-1, 3).tolist()] + ['']
    assert len(got) == len(want)
    wrong = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not wrong, (len(wrong), wrong[:5])


def test_vertices_keep_offset_colours_and_declined_rows():
    xyz = np.array([[0.5, -0.0, 1e-7], [1, 2, 3], [np.inf, 0, 0], [0, 2.0**31, 0], [7, 8, 9], [-1e-9, 1e9, 4]], np.float32)
    off = np.full((6, 3), 0.25, np.float32)
    rgb = np.array([[0, 9, 10], [99, 100, 255], [1, 1, 1], [2, 2, 2], [3, 3, 3], [4, 40, 140]], np.uint8)
    keep = np.array([1, 0, 1, 1, 0, 1], np.uint8)
    text, lines, declined, dropped = ply_vertices(xyz, rgb, keep, off)
    s = (xyz + off).astype(np.float64)
    want = ''.join('%f %f %f %d %d %d\n' % (tuple(s[i]) + tuple(rgb[i])) for i in (0, 5))
    assert (text.decode(), lines, declined, dropped) == (want, 2, 2, 0)
    text, lines, declined, dropped = ply_vertices(xyz[:0])
    assert (text, lines, declined) == (b'', 0, 0)


def random_masks(rng, n, n_inst, runs_per_mask=12, longest=4000):
    masks = np.zeros((n_inst, n), np.uint8)
    for k in range(n_inst):
        for _ in range(int(rng.integers(0, runs_per_mask))):
            lo = int(rng.integers(0, n))
            masks[k, lo:lo + int(rng.integers(1, longest))] = 1
    masks[0, :] = 0                                    # an empty mask
    masks[1, -1] = 1                                   # the last point
    masks[2, 31:33] = 1                                # across a word
    return masks


def runs_of(masks):
    starts, ends, bounds = [], [], [0]
    for m in masks:
        p = np.concatenate([[0], m, [0]]).astype(np.int8)
        e = np.flatnonzero(p[1:] != p[:-1])
        starts += e[0::2].tolist()
        ends += e[1::2].tolist()
        bounds.append(len(starts))
    return np.array(starts, np.int32), np.array(ends, np.int32), np.array(bounds, np.int64)


def bit_rows(masks):
    n_inst, n = masks.shape
    words = (n + 31) // 32
    padded = np.ones((n_inst, words * 32), np.uint8)  # (bits beyond n are set: the kernels must ignore them)
    padded[:, :n] = masks
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder='little')).view(np.int32).reshape(n_inst, words)


def paint(masks, priority, skip, form):
    lib = L.lib()
    n_inst, n = masks.shape
    label = torch.full((max(n, 1), ), 7, dtype=torch.int32, device='cuda')
    pointnum = torch.full((max(n_inst, 1), ), -7, dtype=torch.int32, device='cuda')
    pd, sd = dev(priority, np.int32), dev(skip, np.uint8)
    if form == 'bits':
        bd = dev(bit_rows(masks))
        L.check(lib.sg_viz_paint_bits(L.ptr(bd), n_inst, n, L.ptr(pd), L.ptr(sd), L.ptr(label), L.ptr(pointnum),
                                      L.stream()), 'sg_viz_paint_bits')
    else:
        s, e, b = runs_of(masks)
        s_d, e_d, b_d = dev(s), dev(e), dev(b)
        ws = L.workspace(lib.sg_viz_paint_runs_workspace_bytes(n_inst, n), 'cuda')
        L.check(lib.sg_viz_paint_runs(L.ptr(s_d), L.ptr(e_d), L.ptr(b_d), len(s), n_inst, n, L.ptr(pd), L.ptr(sd),
                                      L.ptr(label), L.ptr(pointnum), L.ptr(ws), ws.numel(), L.stream()),
                'sg_viz_paint_runs')
    return label[:n].cpu().numpy(), pointnum[:n_inst].cpu().numpy()


def dense_paint(masks, priority, skip):
    n_inst, n = masks.shape
    label = np.full(n, -100, np.int32)
    for k in sorted(range(n_inst), key=lambda k: (priority[k], k)):       # ascending: the last write wins
        if not skip[k]:
            label[masks[k] == 1] = k
    return label, np.where(skip, 0, masks.sum(axis=1)).astype(np.int32)


@pytest.mark.parametrize('n,n_inst', [(150000, 100), (4099, 7), (33, 3)])
def test_paint_from_bits_and_runs_equals_dense_numpy(n, n_inst):
    rng = np.random.default_rng(n)
    masks = random_masks(rng, n, n_inst, longest=max(n // 30, 2))
    priority = rng.permutation(n_inst)
    priority[n_inst // 2] = priority[0]                 # a tie: the higher index wins
    skip = rng.random(n_inst) < 0.15
    want = dense_paint(masks, priority, skip)
    for form in ('bits', 'runs'):
        label, pointnum = paint(masks, priority, skip, form)
        assert np.array_equal(label, want[0]), form
        assert np.array_equal(pointnum, want[1]), form


def test_instance_rank_rule():
    lib = L.lib()
    rng = np.random.default_rng(3)
    for counts in ([5, 9, 5, 0, 9, 0], rng.integers(0, 40, size=999), [3], rng.integers(0, 2**31 - 1, size=3000)):
        counts = np.asarray(counts, np.int32)
        n = len(counts)
        rank = torch.full((n, ), -1, dtype=torch.int32, device='cuda')
        ws = L.workspace(lib.sg_viz_instance_rank_workspace_bytes(n), 'cuda')
        cd = dev(counts)
        L.check(lib.sg_viz_instance_rank(L.ptr(cd), n, L.ptr(rank), L.ptr(ws), ws.numel(), L.stream()),
                'sg_viz_instance_rank')
        assert np.array_equal(rank.cpu().numpy(), V._rank(counts))
    # by hand: 9 (index 4), 9 (index 1), 5 (index 2), 5 (index 0), 0 (index 5), 0 (index 3)
    assert V._rank(np.array([5, 9, 5, 0, 9, 0])).tolist() == [3, 1, 2, 5, 0, 4]


def test_ties_follow_the_documented_rule_on_the_device(tmp_path):
    check_ties('device', tmp_path)


@pytest.mark.parametrize('name', ['scene0011_00', 'scene0704_01', 'single_kept'])
def test_colors_from_result_equals_the_saved_tree_on_the_device(name, tmp_path):
    check_result_equals_tree(CASES[name], str(tmp_path), 'device')


def test_write_ply_on_the_device(tmp_path):
    for name, args in mg.direct_calls().items():
        p = str(tmp_path / (name + '.ply'))
        info = V.write_ply(*args, p, backend='device')
        assert open(p, 'rb').read() == base64.b64decode(GOLD['write_ply'][name]), name
        assert info['formatted_by'] == ('device' if name == 'faces' else 'numpy')      # (float64 vertices: numpy)


def big_result(n, n_masks, seed):
    rng = np.random.default_rng(seed)
    masks = random_masks(rng, n, n_masks)
    scores = rng.permutation(9000)[:n_masks] / 10000.0 + 0.05
    f3 = lambda s: (rng.standard_normal((n, 3)) * s).astype(np.float32)  # noqa: E731
    label = rng.integers(0, 20, size=n)
    label[rng.random(n) < 0.1] = -100
    inst = rng.integers(0, 60, size=n)
    gt = np.where(rng.random(n) < 0.2, 0, (inst % 18 + 1) * 1000 + inst + 1).astype(np.int64)
    return dict(scan_id='scene_big', coords_float=f3(4.0), color_feats=rng.uniform(-1, 1, (n, 3)).astype(np.float32),
                semantic_labels=label.astype(np.int64), semantic_preds=rng.integers(0, 20, size=n).astype(np.int64),
                offset_preds=f3(0.2), offset_labels=f3(0.2), gt_instances=gt,
                pred_instances=[dict(scan_id='scene_big', label_id=k % 18 + 1, conf=float(scores[k]),
                                     pred_mask=rle_encode(masks[k])) for k in range(n_masks)])


def test_one_scan_end_to_end(tmp_path):
    result = big_result(150000, 100, 8)
    root = str(tmp_path / 'out')
    R.save_results(root, [result], ['semantic', 'instance'], Dataset, backend='device')
    on_dev = V.save_visualizations(root, ['scene_big'], vc.TASKS, str(tmp_path / 'dev'), backend='device')
    on_host = V.save_visualizations(root, ['scene_big'], vc.TASKS, str(tmp_path / 'np'), backend='numpy')
    kept = int((result['semantic_labels'] != -100).sum())
    for d, h in zip(on_dev, on_host):
        assert d['formatted_by'] == 'device' and d['declined'] == 0 and d['vertices'] == h['vertices'] == kept
        a, b = open(d['path'], 'rb').read(), open(h['path'], 'rb').read()
        assert len(a) == d['bytes'] and a == b, d['task']
    a = V.colors_from_result(result, 'instance_pred', backend='device')
    b = V.get_coords_color(root, 'scene_big', 'instance_pred', backend='numpy')
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
