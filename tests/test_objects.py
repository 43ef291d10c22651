"""The object table of a mask list: the numpy twins of ``softgroup_amd.ops.objects`` against independent brute forces
written here (plain loops with Python floats, ``math.fsum``, a recursive tree), a hand-made case for every rule,
``describe_instances`` end to end, the JSON table and the CLI.  tests/test_objects_gpu.py runs the device on the same
cases."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from softgroup_amd.ops import objects as OB
from softgroup_amd.util import (box_corners, describe_instances, describe_result, load_objects, rle_encode,
                                save_objects, save_results)
from softgroup_amd.util.lazy import LazyResults

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- cases --------------------------------------------------------------------------------------------------------------
def pack(dense):
    """bool [n, N] -> packed uint8 rows [n, ceil(N / 32) * 4]"""
    dense = np.asarray(dense, dtype=bool)
    n, n_points = dense.shape
    rows = np.zeros((n, (n_points + 31) // 32 * 4), np.uint8)
    for m in range(n):
        p = np.packbits(dense[m], bitorder='little')
        rows[m, :p.size] = p
    return rows


def cloud(seed, n_points, kind='normal'):
    """float32 [N, 3]: 'normal' around 0 (negative values), 'far' around 1e4, 'dup' exact duplicates, 'lattice' a grid
    (many equal extremes)"""
    rng = np.random.default_rng(seed)
    if kind == 'far':
        return (1e4 + rng.standard_normal((n_points, 3)) * 3).astype(np.float32)
    if kind == 'dup':
        base = (rng.standard_normal((max(n_points // 7, 1), 3)) * 4).astype(np.float32)
        return base[rng.integers(base.shape[0], size=n_points)]
    if kind == 'lattice':
        return rng.integers(-3, 4, size=(n_points, 3)).astype(np.float32) * np.float32(0.25)
    return (rng.standard_normal((n_points, 3)) * 4 - 1).astype(np.float32)


def masks(seed, n, n_points, density):
    """bool [n, N]: ``density`` a fraction, 'all', or 'last' (mask 0 confined to the last word)"""
    rng = np.random.default_rng(seed)
    if density == 'all':
        return np.ones((n, n_points), bool)
    if density == 'last':
        dense = rng.random((n, n_points)) < 0.5
        dense[0] = False
        dense[0, (n_points - 1) // 32 * 32:] = True
        return dense
    dense = rng.random((n, n_points)) < density
    dense[:, rng.integers(n_points)] = True                 # (no mask is empty by accident)
    return dense


# ---- brute forces ------------------------------------------------------------------------------------------------------
def brute_extents(coords, member, table):
    """one mask: plain loops with Python floats -> (ext [A, 4], best index)"""
    pts = [(float(x), float(y)) for x, y in coords[member][:, :2]]
    ext, best, best_area = [], -1, None
    for c, s in [(float(c), float(s)) for c, s in table]:
        us = [x * c + y * s for x, y in pts]
        vs = [y * c - x * s for x, y in pts]
        e = [min(us) + 0.0, max(us) + 0.0, min(vs) + 0.0, max(vs) + 0.0]
        area = (e[1] - e[0]) * (e[3] - e[2])
        if best < 0 or area < best_area:
            best, best_area = len(ext), area
        ext.append(e)
    return np.array(ext, np.float64), best


def brute_obb(ext, c, s, theta, zmin, zmax):
    umin, umax, vmin, vmax = (float(v) for v in ext)
    c, s, zmin, zmax = float(c), float(s), float(zmin), float(zmax)
    uc, vc = (umin + umax) * 0.5, (vmin + vmax) * 0.5
    return np.array([uc * c - vc * s, uc * s + vc * c, (zmin + zmax) * 0.5, umax - umin, vmax - vmin, zmax - zmin,
                     float(theta)], np.float64)


def slow_sum(values, member):
    """the definition, slowly: values float64 [N] -> the leaf of every word by a loop, the tree by recursion"""
    n_points = member.size
    words = (n_points + 31) // 32
    leaves = []
    for w in range(words):
        acc = 0.0
        for b in range(32):
            i = 32 * w + b
            if i < n_points and member[i]:
                acc = acc + float(values[i])
        leaves.append(acc)
    size = 1
    while size < words:
        size *= 2
    leaves += [0.0] * (size - words)

    def tree(a):
        return a[0] if len(a) == 1 else tree(a[:len(a) // 2]) + tree(a[len(a) // 2:])

    return tree(leaves) if leaves else 0.0


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- extents and boxes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['normal', 'far', 'dup', 'lattice'])
@pytest.mark.parametrize('yaw_steps', [1, 7, 90])
def test_extents_and_boxes_equal_the_plain_loop(kind, yaw_steps):
    n_points, n = 333, 4
    coords = cloud(3, n_points, kind)
    dense = masks(4, n, n_points, 0.2)
    theta, table = OB.yaw_table(yaw_steps)
    got = OB.instance_extents_numpy(pack(dense), n_points, coords, table)
    assert got['flags'] == 0
    insts = [dict(pred_mask=dense[m]) for m in range(n)]
    obb = describe_instances(insts, coords, yaw_steps=yaw_steps, backend='numpy')
    for m in range(n):
        ext, best = brute_extents(coords, dense[m], table)
        assert bits_equal(got['all_ext'][m], ext)
        assert got['best_index'][m] == best and obb['angle_index'][m] == best
        assert bits_equal(got['best_ext'][m], ext[best])
        z = coords[dense[m], 2].astype(np.float64)
        want = brute_obb(ext[best], table[best, 0], table[best, 1], theta[best], z.min() + 0.0, z.max() + 0.0)
        assert bits_equal(obb['obb'][m], want)


def test_per_mask_tables_equal_the_plain_loop():
    n_points, n, r = 200, 3, 2
    coords = cloud(5, n_points)
    dense = masks(6, n, n_points, 0.3)
    tabs = OB.refine_tables(12, r)[1][[0, 5, 11]]
    got = OB.instance_extents_numpy(pack(dense), n_points, coords, tabs, 2 * r + 1)
    for m in range(n):
        ext, best = brute_extents(coords, dense[m], tabs[m])
        assert bits_equal(got['all_ext'][m], ext) and got['best_index'][m] == best


def test_refined_area_is_never_larger():
    n_points, n = 400, 6
    coords = cloud(7, n_points)
    insts = [dict(pred_mask=d) for d in masks(8, n, n_points, 0.1)]
    coarse = describe_instances(insts, coords, yaw_steps=9, backend='numpy')
    fine = describe_instances(insts, coords, yaw_steps=9, refine=8, backend='numpy')
    assert np.array_equal(coarse['angle_index'], fine['angle_index'])
    assert (fine['obb'][:, 3] * fine['obb'][:, 4] <= coarse['obb'][:, 3] * coarse['obb'][:, 4]).all()


# ---- sums ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_points', [1, 31, 33, 1000, 4097])
def test_sums_equal_the_recursive_tree_byte_for_byte(n_points):
    coords, colors = cloud(9, n_points, 'far'), cloud(10, n_points)
    dense = masks(11, 2, n_points, 0.5)
    got = OB.instance_moments_numpy(pack(dense), n_points, coords, colors)
    for m in range(2):
        count = float(dense[m].sum())
        sums = [slow_sum(coords[:, k].astype(np.float64), dense[m]) for k in range(3)]
        assert bits_equal(got['sum_xyz'][m], sums)
        cen = [s / count for s in sums]
        assert bits_equal(got['centroid'][m], cen)
        d = [[float(x) - cen[k] for x in coords[:, k]] for k in range(3)]
        pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
        cov = [slow_sum(np.array([a * b for a, b in zip(d[i], d[j])]), dense[m]) / count for i, j in pairs]
        assert bits_equal(got['cov6'][m], cov)
        col = [slow_sum(colors[:, k].astype(np.float64), dense[m]) / count for k in range(3)]
        assert bits_equal(got['mean_color'][m], col)
        own = coords[dense[m]].astype(np.float64)
        assert bits_equal(got['aabb'][m], np.concatenate([own.min(0), own.max(0)]) + 0.0)
        assert got['npoint'][m] == dense[m].sum()


def test_sums_within_the_first_order_bound_of_fsum():
    """|twin - fsum| <= (32 + ceil(log2 W)) * 2^-53 * 1.01 * sum|v|: 32 sequential additions plus the tree's depth"""
    n_points = 100003
    coords = cloud(12, n_points, 'far')
    dense = masks(13, 2, n_points, 0.5)
    got = OB.instance_moments_numpy(pack(dense), n_points, coords)
    words = (n_points + 31) // 32
    for m in range(2):
        own = coords[dense[m]].astype(np.float64)
        for k in range(3):
            exact = math.fsum(own[:, k].tolist())
            bound = (32 + math.ceil(math.log2(words))) * 2.0 ** -53 * 1.01 * math.fsum(np.abs(own[:, k]).tolist())
            err = abs(float(got['sum_xyz'][m, k]) - exact)
            print(f'mask {m} axis {k}: error {err:.3e}, bound {bound:.3e}')
            assert err <= bound
        cen = got['centroid'][m]
        d = own - cen[None, :]
        for q, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            v = d[:, i] * d[:, j]
            exact = math.fsum(v.tolist())
            bound = (32 + math.ceil(math.log2(words))) * 2.0 ** -53 * 1.01 * math.fsum(np.abs(v).tolist())
            err = abs(float(got['cov6'][m, q]) * own.shape[0] - exact)
            # (the division and the multiplication back cost one rounding each of the total)
            assert err <= bound + 2 * 2.0 ** -53 * abs(exact)


# ---- the known rectangle ---------------------------------------------------------------------------------------------------
def rectangle(degrees):
    rng = np.random.default_rng(14)
    local = np.concatenate([np.array([[-2, -0.5], [2, -0.5], [2, 0.5], [-2, 0.5]], np.float64),
                            rng.uniform([-1.99, -0.49], [1.99, 0.49], size=(200, 2))])
    t = math.radians(degrees)
    xy = np.stack([3 + local[:, 0] * math.cos(t) - local[:, 1] * math.sin(t),
                   -2 + local[:, 0] * math.sin(t) + local[:, 1] * math.cos(t)], axis=1)
    return np.concatenate([xy, rng.uniform(0, 1.5, size=(204, 1))], axis=1).astype(np.float32)


def test_known_rectangle():
    """coordinates stay below 10, where float32 numbers are 9.5e-7 apart; an extent is at most four roundings off"""
    coords = rectangle(30.0)
    insts = [dict(pred_mask=np.ones(204, bool))]
    t = describe_instances(insts, coords, yaw_steps=90, backend='numpy')
    assert t['angle_index'][0] == 30
    assert abs(t['obb'][0, 3] - 4) <= 1e-5 and abs(t['obb'][0, 4] - 1) <= 1e-5
    assert abs(t['obb'][0, 0] - 3) <= 1e-5 and abs(t['obb'][0, 1] + 2) <= 1e-5
    assert t['obb'][0, 6] == 30 * (np.pi / 2) / 90
    corners = box_corners(t)
    assert corners.shape == (1, 8, 3)
    for x, y in coords[:4, :2].astype(np.float64):
        assert np.hypot(corners[0, :4, 0] - x, corners[0, :4, 1] - y).min() <= 2e-5
    assert corners[0, :4, 2].tolist() == [t['aabb'][0, 2]] * 4 and corners[0, 4:, 2].tolist() == [t['aabb'][0, 5]] * 4
    coords = rectangle(30.5)
    t = describe_instances(insts, coords, yaw_steps=90, refine=1, backend='numpy')
    assert t['angle_index'][0] in (30, 31)
    assert abs(t['obb'][0, 6] - math.radians(30.5)) <= 1e-12
    assert abs(t['obb'][0, 3] - 4) <= 1e-5 and abs(t['obb'][0, 4] - 1) <= 1e-5


def test_one_yaw_step_is_the_axis_aligned_box():
    coords = cloud(15, 500)
    dense = masks(16, 3, 500, 0.2)
    t = describe_instances([dict(pred_mask=d) for d in dense], coords, yaw_steps=1, backend='numpy')
    a = t['aabb']
    want = np.stack([(a[:, 0] + a[:, 3]) * 0.5, (a[:, 1] + a[:, 4]) * 0.5, (a[:, 2] + a[:, 5]) * 0.5,
                     a[:, 3] - a[:, 0], a[:, 4] - a[:, 1], a[:, 5] - a[:, 2], np.zeros(3)], axis=1)
    assert bits_equal(t['obb'], want + 0.0) and (t['angle_index'] == 0).all()


# ---- ties, zero sign, empty inputs -----------------------------------------------------------------------------------------
def test_tie_rules():
    coords = np.array([[1, 1, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], np.float32)
    dense = np.array([[0, 0, 0, 0, 1],                    # a single point: every area is 0
                      [1, 1, 1, 1, 0],                    # a square
                      [1, 1, 0, 0, 1]], bool)             # shares points with both
    t = describe_instances([dict(pred_mask=d) for d in dense], coords, semantic=np.array([3, 1, 1, 3, 7]),
                           n_classes=6, yaw_steps=90, backend='numpy')
    assert t['angle_index'].tolist() == [0, 0, 45]
    assert t['obb'][0, 3:6].tolist() == [0.0, 0.0, 0.0]
    assert t['npoint'].tolist() == [1, 4, 3]
    # mask 0: its only label, 7, is outside 0 .. 5; mask 1: classes 1 and 3 twice each -> 1; mask 2: 3 and 1 once
    assert t['sem_label'].tolist() == [-1, 1, 1] and t['sem_count'].tolist() == [0, 2, 1]
    hist = OB.instance_class_hist_numpy(pack(dense), 5, np.array([3, 1, 1, 3, -1]), 4)
    assert hist['hist'].tolist() == [[0, 0, 0, 0], [0, 2, 0, 2], [0, 1, 0, 1]]


def test_zero_sign_does_not_depend_on_the_point_order():
    a = np.array([[-0.0, -0.0, -0.0], [0.0, 0.0, 0.0]], np.float32)
    for coords in (a, a[::-1].copy()):
        dense = np.ones((1, 2), bool)
        ex = OB.instance_extents_numpy(pack(dense), 2, coords, OB.yaw_table(1)[1])
        mo = OB.instance_moments_numpy(pack(dense), 2, coords)
        assert not np.signbit(ex['all_ext']).any() and not np.signbit(mo['aabb']).any()
        assert bits_equal(ex['best_ext'], np.zeros((1, 4))) and bits_equal(mo['aabb'], np.zeros((1, 6)))


def test_empty_inputs():
    coords = cloud(17, 70)
    dense = np.zeros((2, 70), bool)
    dense[1, 5:9] = True
    t = describe_instances([dict(pred_mask=d) for d in dense], coords, colors=coords, semantic=np.zeros(70, np.int64),
                           n_classes=2, refine=1, backend='numpy')
    assert t['npoint'].tolist() == [0, 4] and t['angle_index'][0] == -1 and t['sem_label'].tolist() == [-1, 0]
    for key in ('aabb', 'centroid', 'cov6', 'obb', 'mean_color'):
        assert np.isnan(t[key][0]).all() and np.isfinite(t[key][1]).all()
    t = describe_instances([], coords, backend='numpy')                                # n = 0
    assert t['npoint'].shape == (0, ) and t['obb'].shape == (0, 7) and t['aabb'].shape == (0, 6)
    t = describe_instances([dict(pred_mask=np.zeros(0, bool))], np.zeros((0, 3), np.float32), backend='numpy')   # N = 0
    assert t['npoint'].tolist() == [0] and np.isnan(t['obb']).all()
    mo = OB.instance_moments_numpy(np.zeros((3, 0), np.uint32), 0, np.zeros((0, 3), np.float32))
    assert mo['npoint'].tolist() == [0, 0, 0] and np.isnan(mo['sum_xyz']).all()


# ---- errors ---------------------------------------------------------------------------------------------------------------
def test_errors():
    coords = cloud(18, 64)
    dense = np.zeros((1, 64), bool)
    dense[0, :10] = True
    insts = [dict(pred_mask=dense[0])]
    for bad in (np.nan, np.inf, -np.inf):
        hit = coords.copy()
        hit[3, 1] = bad
        with pytest.raises(ValueError):
            describe_instances(insts, hit, backend='numpy')
        with pytest.raises(ValueError):
            describe_instances(insts, coords, colors=hit, backend='numpy')
        miss = coords.copy()
        miss[40] = bad                                                                # a point that is in no mask
        describe_instances(insts, miss, colors=miss, backend='numpy')
    for kw in (dict(yaw_steps=0), dict(yaw_steps=181), dict(refine=9), dict(refine=-1),
               dict(semantic=np.zeros(64, np.int64), n_classes=0), dict(semantic=np.zeros(64, np.int64))):
        with pytest.raises(ValueError):
            describe_instances(insts, coords, backend='numpy', **kw)
    with pytest.raises(ValueError):
        describe_instances(insts, coords[:63], backend='numpy')
    with pytest.raises(ValueError):
        describe_instances(insts, coords, backend='cuda')


# ---- table, files, CLI ----------------------------------------------------------------------------------------------------
def test_rle_dicts_and_dense_masks_give_equal_tables():
    coords = cloud(19, 900)
    dense = masks(20, 5, 900, 0.1)
    dense[2] = False
    as_rle = [dict(scan_id='s', label_id=m, conf=0.5 + m / 16, pred_mask=rle_encode(d.astype(np.int64)))
              for m, d in enumerate(dense)]
    as_dense = [dict(i, pred_mask=d) for i, d in zip(as_rle, dense)]
    kw = dict(colors=cloud(21, 900), semantic=np.arange(900) % 5, n_classes=5, refine=2, backend='numpy')
    a, b = describe_instances(as_rle, coords, **kw), describe_instances(as_dense, coords, **kw)
    assert sorted(a) == sorted(['npoint', 'aabb', 'centroid', 'cov6', 'obb', 'angle_index', 'mean_color',
                                'sem_label', 'sem_count', 'scan_id', 'label_id', 'conf'])
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key
    assert a['label_id'].tolist() == [0, 1, 2, 3, 4] and a['conf'][4] == 0.75 and a['scan_id'][0] == 's'
    res = LazyResults(pred_instances=as_rle, coords_float=coords, color_feats=kw['colors'],
                      semantic_preds=kw['semantic'])
    c = describe_result(res, n_classes=5, refine=2, backend='numpy')
    for key in a:
        assert a[key].tobytes() == c[key].tobytes(), key


def test_save_and_load_round_trip(tmp_path):
    coords = cloud(22, 300, 'far')
    dense = masks(23, 4, 300, 0.3)
    dense[1] = False                                                                    # a NaN row
    insts = [dict(scan_id='room', label_id=3, conf=0.1 * m, pred_mask=d) for m, d in enumerate(dense)]
    t = describe_instances(insts, coords, colors=coords, semantic=np.arange(300) % 3, n_classes=3, backend='numpy')
    path = str(tmp_path / 'room.objects.json')
    save_objects(path, t)
    text = open(path).read()
    assert 'NaN' not in text and 'null' in text
    back = load_objects(path)
    assert sorted(back) == sorted(t)
    for key in t:
        assert back[key].dtype == t[key].dtype and back[key].shape == t[key].shape, key
        assert back[key].tobytes() == t[key].tobytes(), key


class _Dataset:
    NYU_ID = None


def test_cli_on_a_saved_tree(tmp_path):
    n_points = 500
    coords, colors = cloud(24, n_points), cloud(25, n_points)
    dense = masks(26, 3, n_points, 0.2)
    semantic = (np.arange(n_points) % 4).astype(np.int64)
    insts = [dict(scan_id='room_a', label_id=1 + m, conf=0.25 * (m + 1), pred_mask=rle_encode(d.astype(np.int64)))
             for m, d in enumerate(dense)]
    zeros = np.zeros((n_points, 3), np.float32)
    result = dict(scan_id='room_a', coords_float=coords, color_feats=colors, semantic_preds=semantic,
                  semantic_labels=semantic, offset_preds=zeros, offset_labels=zeros, pred_instances=insts,
                  gt_instances=np.zeros(n_points, np.int64))
    out = str(tmp_path / 'results')
    save_results(out, [result], ['semantic', 'instance'], _Dataset, backend='numpy')
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'objects.py'), '--prediction_path', out, '--all-rooms',
           '--out-dir', str(tmp_path / 'objects'), '--n-classes', '4', '--refine', '1', '--backend', 'numpy']
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    got = load_objects(str(tmp_path / 'objects' / 'room_a.objects.json'))
    want = describe_instances(insts, coords, colors, semantic, 4, refine=1, backend='numpy')
    for key in ('npoint', 'aabb', 'centroid', 'cov6', 'obb', 'angle_index', 'mean_color', 'sem_label', 'sem_count',
                'label_id'):
        assert got[key].tobytes() == want[key].tobytes(), key
