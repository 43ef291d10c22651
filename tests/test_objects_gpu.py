"""The HIP kernels of csrc/objects.hip and the device path of ``describe_instances`` against the numpy twins of
``softgroup_amd.ops.objects`` on the cases of tests/test_objects.py: device equals twin byte for byte (floats compared
through their uint64 views), two calls give equal bytes."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from softgroup_amd import _lib as L
from softgroup_amd import synthetic
from softgroup_amd.ops import objects as OB
from softgroup_amd.util import describe_instances, ensemble_results, rle_encode, stitch_results

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_objects import cloud, masks, pack  # noqa: E402

pytestmark = pytest.mark.gpu


def _csrc():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'softgroup_amd', 'csrc',
                        'objects.hip')
    with open(path) as f:
        return f.read()


def _const(name):
    m = re.search(r'constexpr\s+int\s+' + name + r'\s*=\s*(\d+)\s*;', _csrc())
    assert m, f'constexpr int {name} not found'
    return int(m.group(1))


CHUNK_POINTS = 32 * _const('kObjChunkWords')
N_EDGES = (1, 31, 32, 33, 63, 65, 2049, 70001, CHUNK_POINTS + 1, 2 * CHUNK_POINTS + 33)
MASK_COUNTS = (1, 7, 9, 33)
DENSITIES = (0.01, 0.5, 'all', 'last')
KINDS = ('normal', 'far', 'dup', 'lattice')


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared inputs are read-only)


def words(rows, n_points):
    rows = np.ascontiguousarray(rows)
    return dev(rows.view(np.int32).reshape(rows.shape[0], (n_points + 31) // 32))


def same_bytes(got, want, key=''):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (key, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), key


def check_moments(rows, n_points, coords, colors=None):
    want = OB.instance_moments_numpy(rows, n_points, coords, colors)
    args = (words(rows, n_points), n_points, dev(coords), None if colors is None else dev(colors))
    got, again = OB.instance_moments(*args), OB.instance_moments(*args)
    assert int(got['flags'].item()) == want['flags'] == 0
    for key in want:
        if key != 'flags':
            same_bytes(got[key], want[key], key)
            same_bytes(again[key], want[key], key)


def check_extents(rows, n_points, coords, table, row_stride=0):
    want = OB.instance_extents_numpy(rows, n_points, coords, table, row_stride)
    args = (words(rows, n_points), n_points, dev(coords), dev(table), row_stride)
    got, again = OB.instance_extents(*args, all_extents=True), OB.instance_extents(*args, all_extents=True)
    lean = OB.instance_extents(*args)                                # the keys in the workspace
    assert int(got['flags'].item()) == want['flags'] == 0 and 'all_ext' not in lean
    for key in ('all_ext', 'best_index', 'best_ext'):                 # (all_ext first: it localises a failure)
        same_bytes(got[key], want[key], key)
        same_bytes(again[key], want[key], key)
        if key != 'all_ext':
            same_bytes(lean[key], want[key], key)
    # the best row is the twin's selection from all extremes
    idx = want['best_index']
    some = idx >= 0
    all_ext = got['all_ext'].cpu().numpy()
    assert np.array_equal(all_ext[some, idx[some]].view(np.uint64), got['best_ext'].cpu().numpy()[some].view(np.uint64))


# ---- sizes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_points', N_EDGES)
def test_moments_device_equals_twin(n_points):
    n = MASK_COUNTS[N_EDGES.index(n_points) % 4] if n_points <= 2049 else 7
    coords, colors = cloud(n_points, n_points, KINDS[N_EDGES.index(n_points) % 4]), cloud(n_points + 1, n_points)
    for density in DENSITIES:
        dense = masks(n_points + 2, n, n_points, density)
        if density == 0.5 and n > 1:
            dense[n // 2] = False                                     # an empty mask among the others
        check_moments(pack(dense), n_points, coords, colors)
    check_moments(pack(masks(n_points + 3, n, n_points, 0.5)), n_points, coords)          # without colours


@pytest.mark.parametrize('n_points', N_EDGES)
def test_extents_device_equals_twin(n_points):
    n = MASK_COUNTS[(N_EDGES.index(n_points) + 1) % 4] if n_points <= 2049 else 7
    coords = cloud(n_points + 4, n_points, KINDS[(N_EDGES.index(n_points) + 2) % 4])
    table = OB.yaw_table(90 if n_points <= 2049 else 9)[1]
    for density in DENSITIES:
        dense = masks(n_points + 5, n, n_points, density)
        if density == 0.5 and n > 1:
            dense[0] = False
        check_extents(pack(dense), n_points, coords, table)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n', MASK_COUNTS)
def test_mask_counts_and_coordinates(n, kind):
    n_points = 2049
    coords = cloud(n, n_points, kind)
    rows = pack(masks(n + 1, n, n_points, 0.01 if n == 33 else 0.5))
    check_moments(rows, n_points, coords, coords)
    check_extents(rows, n_points, coords, OB.yaw_table(7)[1])


# ---- angle counts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_angles', [1, 2, 7, 90, 180])
def test_angle_counts_with_shared_and_per_mask_tables(n_angles):
    n_points, n = CHUNK_POINTS + 77, 9
    coords = cloud(n_angles, n_points)
    rows = pack(masks(n_angles + 1, n, n_points, 0.5))
    theta, table = OB.yaw_table(n_angles)
    check_extents(rows, n_points, coords, table)
    rng = np.random.default_rng(n_angles)
    own = theta[None, :] + rng.uniform(0, 0.01, size=(n, 1))
    check_extents(rows, n_points, coords, np.stack([np.cos(own), np.sin(own)], axis=-1), n_angles)


@pytest.mark.parametrize('refine', [0, 1, 8])
def test_refine(refine):
    n_points, n = 3000, 9
    coords = cloud(40 + refine, n_points, 'far')
    dense = masks(41, n, n_points, 0.1)
    dense[4] = False
    insts = [dict(label_id=m, conf=0.5, pred_mask=rle_encode(d.astype(np.int64))) for m, d in enumerate(dense)]
    want = describe_instances(insts, coords, yaw_steps=90, refine=refine, backend='numpy')
    got = describe_instances(insts, coords, yaw_steps=90, refine=refine, backend='device')
    assert sorted(got) == sorted(want)
    for key in want:
        same_bytes(got[key], want[key], key)


# ---- above the launch cap -------------------------------------------------------------------------------------------------
def test_sixteen_thousand_masks():
    n, n_points = OB.MAX_INSTANCES, 64
    assert _const('kObjMaxInst') == n and n > _const('kObjMaxBlocks')
    rng = np.random.default_rng(50)
    dense = rng.random((n, n_points)) < 0.3
    dense[::97] = False
    coords = cloud(51, n_points)
    rows = pack(dense)
    check_moments(rows, n_points, coords, coords)
    check_extents(rows, n_points, coords, OB.yaw_table(7)[1])
    sem = rng.integers(-1, 5, n_points)
    want = OB.instance_class_hist_numpy(rows, n_points, sem, 4)
    got = OB.instance_class_hist(words(rows, n_points), n_points, dev(sem), 4)
    for key in want:
        same_bytes(got[key], want[key], key)
    with pytest.raises(L.SoftGroupHipError):
        OB.instance_moments(torch.zeros((n + 1, 2), dtype=torch.int32, device='cuda'), n_points, dev(coords))


def test_more_mask_chunks_than_the_grid_cap():
    src = _csrc()
    assert len(re.findall(r'grid_for\(static_cast<int64_t>\(n\) \* (?:a\.)?chunks, 1, kObjMaxBlocks\)', src)) == 3
    cap = _const('kObjMaxBlocks')
    n = 65
    chunks = cap // n + 2
    n_points = chunks * CHUNK_POINTS - 5
    assert n * chunks > cap
    rng = np.random.default_rng(52)
    dense = np.zeros((n, n_points), bool)
    for m in range(n):                                    # a run of points and strays: most chunks are empty
        lo = int(rng.integers(n_points - 3000))
        dense[m, lo:lo + 3000] = rng.random(3000) < 0.7
        dense[m, rng.integers(n_points, size=20)] = True
    dense[7, -1] = True
    coords = cloud(53, n_points)
    rows = pack(dense)
    check_moments(rows, n_points, coords)
    check_extents(rows, n_points, coords, OB.yaw_table(5)[1])
    sem = rng.integers(0, 9, n_points).astype(np.int32)
    want = OB.instance_class_hist_numpy(rows, n_points, sem, 9)
    got = OB.instance_class_hist(words(rows, n_points), n_points, dev(sem), 9)
    for key in want:
        same_bytes(got[key], want[key], key)


# ---- classes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.int32, np.int64])
@pytest.mark.parametrize('n_classes', [1, 20, 256])
def test_class_hist_device_equals_twin(n_classes, dtype):
    n_points, n = CHUNK_POINTS + 33, 9
    rng = np.random.default_rng(n_classes)
    sem = rng.integers(-3, n_classes + 3, n_points).astype(dtype)
    if dtype == np.int64:
        sem[::5] += 2**32                                             # (the low word alone would be in range)
    dense = masks(60, n, n_points, 0.5)
    dense[3] = False
    dense[5] = sem >= n_classes                                       # a mask without a counted label
    rows = pack(dense)
    want = OB.instance_class_hist_numpy(rows, n_points, sem, n_classes)
    args = (words(rows, n_points), n_points, dev(sem), n_classes)
    got, again = OB.instance_class_hist(*args), OB.instance_class_hist(*args)
    assert want['sem_label'][3] == -1 and want['sem_label'][5] == -1 and want['sem_count'][5] == 0
    for key in want:
        same_bytes(got[key], want[key], key)
        same_bytes(again[key], want[key], key)
    with pytest.raises(L.SoftGroupHipError):
        OB.instance_class_hist(args[0], n_points, args[2], 257)


# ---- non-finite values -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
def test_flags_of_values_that_are_not_finite(bad):
    n_points = 5000
    coords = cloud(70, n_points)
    dense = masks(71, 3, n_points, 0.5)
    dense[:, 4500] = False
    dense[1, 4400] = True
    rows, table = words(pack(dense), n_points), OB.yaw_table(7)[1]
    miss = coords.copy()
    miss[4500] = bad                                                  # a point that is in no mask
    assert int(OB.instance_moments(rows, n_points, dev(miss), dev(miss))['flags'].item()) == 0
    assert int(OB.instance_extents(rows, n_points, dev(miss), table)['flags'].item()) == 0
    for axis in (0, 1, 2):
        hit = coords.copy()
        hit[4400, axis] = bad
        assert int(OB.instance_moments(rows, n_points, dev(hit))['flags'].item()) == OB.FLAG_NOT_FINITE
        assert int(OB.instance_moments(rows, n_points, dev(coords), dev(hit))['flags'].item()) == OB.FLAG_NOT_FINITE
        assert int(OB.instance_extents(rows, n_points, dev(hit), table)['flags'].item()) == \
            (OB.FLAG_NOT_FINITE if axis < 2 else 0)
    insts = [dict(pred_mask=d) for d in dense]
    with pytest.raises(ValueError):
        describe_instances(insts, hit, backend='device')
    describe_instances(insts, miss, colors=miss, backend='device')


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def scene_list(n_points=20000, n_masks=40, seed=3):
    xyz, rgb, inst = synthetic.scene_s2(seed=seed, n=n_points)
    n_points = xyz.shape[0]
    rng = np.random.default_rng(seed)
    n_obj = int(inst.max()) + 1
    insts = []
    for k in range(n_masks):
        objs = rng.choice(n_obj, size=2 if k % 5 == 4 else 1, replace=False)
        m = np.isin(inst, objs) & (rng.random(n_points) < 0.9)
        m[rng.integers(n_points, size=30)] = True
        insts.append(dict(scan_id='s', label_id=int(1 + objs[0] % 18), conf=float(f'{rng.uniform():.4f}'),
                          pred_mask=rle_encode(m.astype(np.int64))))
    sem = (np.maximum(inst, 0) % 18).astype(np.int64)
    return np.ascontiguousarray(xyz, dtype=np.float32), np.ascontiguousarray(rgb, dtype=np.float32), sem, insts


def same_tables(got, want):
    assert sorted(got) == sorted(want)
    for key in want:
        same_bytes(got[key], want[key], key)


def test_describe_instances_device_equals_numpy(monkeypatch):
    xyz, rgb, sem, insts = scene_list()
    kw = dict(colors=rgb, semantic=sem, n_classes=18, yaw_steps=90, refine=2)
    want = describe_instances(insts, xyz, backend='numpy', **kw)
    got = describe_instances(insts, xyz, backend='device', **kw)
    same_tables(got, want)
    assert (want['npoint'] > 0).all() and np.isfinite(want['obb']).all()
    # CUDA inputs, dense masks
    dense = [dict(i, pred_mask=_dense(i['pred_mask'])) for i in insts]
    got = describe_instances(dense, dev(xyz), colors=dev(rgb), semantic=dev(sem), n_classes=18, yaw_steps=90, refine=2,
                             backend='device')
    same_tables(got, want)
    # RLE runs that are not ascending: 'device' raises, 'auto' takes numpy whatever _AUTO says
    odd = [dict(label_id=1, conf=0.5, pred_mask=dict(length=8, counts='7 2 1 2'))]
    pts = cloud(80, 8)
    want = describe_instances(odd, pts, backend='numpy')
    assert want['npoint'].tolist() == [4]
    with pytest.raises(ValueError):
        describe_instances(odd, pts, backend='device')
    monkeypatch.setitem(OB._AUTO, 'describe', 'device')
    same_tables(describe_instances(odd, pts, backend='auto'), want)
    same_tables(describe_instances(insts, xyz, backend='auto', **kw),
                describe_instances(insts, xyz, backend='numpy', **kw))


def _dense(rle):
    from softgroup_amd.util import rle_decode
    return rle_decode(rle).astype(bool)


def test_stitched_and_ensembled_results_go_through():
    from test_ensemble import e2e_case as ensemble_case
    from test_stitch import E2E_CASES, e2e_case as stitch_case
    xyz, _, sem, tiles, results = stitch_case(*E2E_CASES[0])
    out = stitch_results(results, tiles, coords=xyz, gt=dict(semantic_labels=sem), backend='device')
    assert out['pred_instances'] and all(isinstance(i['pred_mask'], dict) for i in out['pred_instances'])
    xyz = np.ascontiguousarray(xyz.cpu().numpy() if torch.is_tensor(xyz) else xyz, dtype=np.float32)
    same_tables(describe_instances(out['pred_instances'], xyz, backend='device'),
                describe_instances(out['pred_instances'], xyz, backend='numpy'))
    results, kw = ensemble_case('three_pass')
    out = ensemble_results(results, backend='device', **kw)
    pts = cloud(81, 97)
    assert out['pred_instances']
    same_tables(describe_instances(out['pred_instances'], pts, refine=1, backend='device'),
                describe_instances(out['pred_instances'], pts, refine=1, backend='numpy'))
