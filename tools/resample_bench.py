"""Cost of thinning a cloud and of carrying a result back (softgroup_amd.ops.resample, util.propagate_result) on two
synthetic clouds: a 1 M-point S3DIS-like room (walls, floor, ceiling and furniture boxes, 10 x 8 x 3 m) and a
600 k-point STPLS3D-like block (ground, roofs and trees over 120 x 120 m).

Timed, each the median of --reps runs after a warm-up, all in one run:
  voxel downsample at 0.02 and 0.05, both picks
      device_kernel_ms  sg_grid_downsample alone on a resident cloud, from HIP events
      device_wall_ms    ops.resample.grid_downsample (with its read-back of the voxel count), wall time to a synchronise
      numpy_wall_ms     grid_downsample_numpy (np.unique(axis=0) + lexsort)
  nearest point from a 0.25 random sample to the full cloud
      build / query kernels from HIP events, nearest_index wall time; the numpy path is the O(N x M) definition
      and is not feasible at these sizes (no number); scipy's cKDTree next to it when scipy is importable,
      labelled: it is NOT tie-exact (it returns any of the equally near sources)
  propagate_result with 100 and 300 masks from the 0.05-thinned cloud to the full cloud
      device_wall_ms / numpy_wall_ms of the whole call (RLE dicts in, RLE dicts out); the strings must be equal
The device and numpy results are compared in the same run (equality).

    python tools/resample_bench.py [--reps 5] [--out profiles/resample_bench.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from softgroup_amd import _lib as L  # noqa: E402
from softgroup_amd.data import random_downsample  # noqa: E402
from softgroup_amd.ops import resample as RS  # noqa: E402
from softgroup_amd.util import propagate_result  # noqa: E402
from softgroup_amd.util.rle import rle_encode  # noqa: E402

VOXELS = [0.02, 0.05]
PICKS = ['first', 'center']
MASKS = [100, 300]


def s3dis_room(n, seed=0):
    rng = np.random.default_rng(seed)
    size = np.array([10.0, 8.0, 3.0])
    p = rng.random((n, 3)) * size
    kind = rng.integers(0, 8, n)
    for axis, k0 in ((0, 0), (1, 2), (2, 4)):          # two faces per axis
        p[kind == k0, axis] = 0.0
        p[kind == k0 + 1, axis] = size[axis]
    box = kind >= 6                                     # furniture: points on small boxes
    centre = rng.random((40, 3)) * size * [1, 1, 0.3]
    which = rng.integers(0, 40, n)
    p[box] = centre[which[box]] + (rng.random((int(box.sum()), 3)) - 0.5) * [1.2, 0.8, 0.9]
    p += rng.normal(0, 0.004, p.shape)
    return (p - size / 2).astype(np.float32)


def stpls3d_block(n, seed=1):
    rng = np.random.default_rng(seed)
    p = np.empty((n, 3))
    p[:, :2] = rng.random((n, 2)) * 120.0
    p[:, 2] = rng.normal(0, 0.05, n)
    roof = (np.floor(p[:, 0] / 15) + np.floor(p[:, 1] / 15)) % 3 == 0
    p[roof, 2] += 6.0 + 3.0 * (np.floor(p[roof, 0] / 15) % 3)
    tree = (~roof) & (rng.random(n) < 0.2)
    p[tree, 2] += rng.random(int(tree.sum())) * 8.0
    return p.astype(np.float32)


def median_wall(fn, reps, sync=True):
    ts = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def median_events(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def raw_downsample(xyz, voxel, pick):
    """sg_grid_downsample on preallocated buffers -> a callable that only launches"""
    lib, n, dev = L.lib(), xyz.size(0), xyz.device
    ids = torch.empty(n, dtype=torch.int32, device=dev)
    inv = torch.empty(n, dtype=torch.int32, device=dev)
    meta = torch.empty(2, dtype=torch.int32, device=dev)
    ws = L.workspace(lib.sg_grid_downsample_workspace_bytes(n), dev)
    pk = RS._PICK[pick]
    return lambda: L.check(lib.sg_grid_downsample(L.ptr(xyz), n, voxel, pk, L.ptr(ids), L.ptr(inv), L.ptr(meta), L.ptr(ws),
                                                  ws.numel(), L.stream()), 'sg_grid_downsample')


def raw_nearest(src, query, cell):
    lib, n_src, n_query, dev = L.lib(), src.size(0), query.size(0), src.device
    grid = L.workspace(lib.sg_nearest_grid_bytes(n_src), dev)
    meta = torch.empty(2, dtype=torch.int32, device=dev)
    index = torch.empty(n_query, dtype=torch.int32, device=dev)
    ws = L.workspace(lib.sg_nearest_query_workspace_bytes(n_query), dev)

    def build():
        L.check(lib.sg_nearest_build(L.ptr(src), n_src, cell, L.ptr(grid), grid.numel(), L.ptr(meta), L.stream()),
                'sg_nearest_build')

    def query_():
        L.check(lib.sg_nearest_query(L.ptr(src), n_src, cell, L.ptr(grid), grid.numel(), L.ptr(query), n_query, -1.0,
                                     L.ptr(index), None, L.ptr(meta), L.ptr(ws), ws.numel(), L.stream()), 'sg_nearest_query')

    return build, query_, index, meta


def instance_list(seed, n_points, n_masks, chunk=500):
    rng = np.random.default_rng(seed)
    n_chunks = max(1, n_points // chunk)
    n_obj = max(2, n_masks // 3)
    owner = rng.integers(0, 2 * n_obj, n_chunks)
    insts = []
    for _ in range(n_masks):
        g = rng.integers(0, n_obj)
        m = np.repeat((owner == g) & (rng.uniform(size=n_chunks) < rng.uniform(0.5, 0.95)), chunk)[:n_points]
        full = np.zeros(n_points, dtype=np.int64)
        full[:m.size] = m
        insts.append(dict(scan_id='s', label_id=int(rng.integers(1, 4)), conf=float(f'{rng.uniform():.4f}'),
                          pred_mask=rle_encode(full)))
    return insts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--scale', type=float, default=1.0, help='fraction of the clouds (rehearsals)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'resample_bench.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'resample_bench needs a GPU: nothing here is measured without one'
    dev = torch.device('cuda')
    reps = args.reps
    clouds = [('s3dis', s3dis_room(int(1000000 * args.scale))), ('stpls3d', stpls3d_block(int(600000 * args.scale)))]
    lines = [f'# tools/resample_bench.py --reps {reps}  ({torch.cuda.get_device_name(0)}); ms, median of {reps} after a '
             'warm-up; kernels from device events, calls by wall clock to a synchronise']
    rows = []

    lines.append(f'# voxel downsample\n{"cloud":8s} {"points":>8s} {"voxel":>6s} {"pick":>6s} {"voxels":>8s} '
                 f'{"device_kernel":>13s} {"device_wall":>11s} {"numpy_wall":>10s}')
    thinned = {}
    for name, xyz in clouds:
        d_xyz = torch.from_numpy(xyz).to(dev)
        for voxel in VOXELS:
            for pick in PICKS:
                ids, inv = RS.grid_downsample(d_xyz, voxel, pick)                      # (warm-up, and the check)
                t0 = time.perf_counter()
                want_ids, want_inv = RS.grid_downsample_numpy(xyz, voxel, pick)
                first_numpy = 1e3 * (time.perf_counter() - t0)
                assert np.array_equal(ids.cpu().numpy(), want_ids) and np.array_equal(inv.cpu().numpy(), want_inv)
                launch = raw_downsample(d_xyz, voxel, pick)
                launch()
                kernel = median_events(launch, reps)
                wall = median_wall(lambda: RS.grid_downsample(d_xyz, voxel, pick), reps)
                numpy_wall = float(np.median([first_numpy] + [
                    median_wall(lambda: RS.grid_downsample_numpy(xyz, voxel, pick), 1, sync=False) for _ in range(reps - 1)]))
                rows.append(dict(op='voxel', cloud=name, points=len(xyz), voxel=voxel, pick=pick, voxels=len(want_ids),
                                 device_kernel_ms=kernel, device_wall_ms=wall, numpy_wall_ms=numpy_wall))
                lines.append(f'{name:8s} {len(xyz):8d} {voxel:6.2f} {pick:>6s} {len(want_ids):8d} {kernel:13.3f} {wall:11.2f} '
                             f'{numpy_wall:10.1f}')
                print(lines[-1], flush=True)
                if voxel == 0.05 and pick == 'center':
                    thinned[name] = (want_ids, want_inv)

    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    lines.append('# nearest point, a 0.25 random sample -> the full cloud.  numpy (the O(N x M) definition): not feasible at '
                 'these sizes, not run.\n# cKDTree (scipy) is NOT tie-exact: it returns any of the equally near sources; '
                 '"differs" counts queries whose index differs\n'
                 f'{"cloud":8s} {"sources":>8s} {"queries":>8s} {"cell":>7s} {"scanned":>8s} {"build_kernel":>12s} '
                 f'{"query_kernel":>12s} {"device_wall":>11s} {"ckdtree_wall":>12s} {"differs":>8s}')
    for name, xyz in clouds:
        ids = np.sort(random_downsample(len(xyz), 0.25, seed=0))
        src, d_src, d_query = xyz[ids], torch.from_numpy(xyz[ids]).to(dev), torch.from_numpy(xyz).to(dev)
        cell = RS.nearest_default_cell(src.min(0), src.max(0), len(src))
        index, scanned = RS.nearest_index(d_src, d_query, return_meta=True)                # (warm-up)
        got = index.cpu().numpy()
        assert (got[ids] == np.arange(len(ids))).all() or len(np.unique(src, axis=0)) < len(src)
        build, query_, raw_index, meta = raw_nearest(d_src, d_query, cell)
        build(), query_()
        assert torch.equal(raw_index.long(), index)
        build_ms, query_ms = median_events(build, reps), median_events(query_, reps)
        wall = median_wall(lambda: RS.nearest_index(d_src, d_query), reps)
        tree_ms, differs = None, None
        if cKDTree is not None:
            t0 = time.perf_counter()
            _, tree_idx = cKDTree(src).query(xyz)
            tree_ms = 1e3 * (time.perf_counter() - t0)
            differs = int((tree_idx != got).sum())
            d_a = ((xyz.astype(np.float64) - src[got]) ** 2).sum(1)
            d_b = ((xyz.astype(np.float64) - src[tree_idx]) ** 2).sum(1)
            assert (d_a <= d_b).all()
        rows.append(dict(op='nearest', cloud=name, sources=len(src), queries=len(xyz), cell=cell, scanned=scanned,
                         build_kernel_ms=build_ms, query_kernel_ms=query_ms, device_wall_ms=wall, ckdtree_wall_ms=tree_ms,
                         ckdtree_differs=differs))
        lines.append(f'{name:8s} {len(src):8d} {len(xyz):8d} {cell:7.4f} {scanned:8d} {build_ms:12.3f} {query_ms:12.3f} '
                     f'{wall:11.2f} ' + (f'{tree_ms:12.1f} {differs:8d}' if tree_ms is not None else
                                         f'{"no scipy":>12s} {"-":>8s}'))
        print(lines[-1], flush=True)

    lines.append('# propagate_result: masks of the 0.05-thinned cloud (pick center) -> the full cloud, RLE dicts in and out\n'
                 f'{"cloud":8s} {"thinned":>8s} {"points":>8s} {"masks":>5s} {"device_wall":>11s} {"numpy_wall":>10s}')
    for c, (name, xyz) in enumerate(clouds):
        ids, inv = thinned[name]
        for n_masks in MASKS:
            res = dict(scan_id='s', semantic_preds=np.zeros(len(ids), np.int64),
                       pred_instances=instance_list(20 + c, len(ids), n_masks))
            a = propagate_result(res, inv, backend='device')                            # (warm-up)
            t0 = time.perf_counter()
            b = propagate_result(res, inv, backend='numpy')
            first_numpy = 1e3 * (time.perf_counter() - t0)
            assert [i['pred_mask'] for i in a['pred_instances']] == [i['pred_mask'] for i in b['pred_instances']]
            wall = median_wall(lambda: propagate_result(res, inv, backend='device'), reps)
            numpy_wall = float(np.median([first_numpy] + [
                median_wall(lambda: propagate_result(res, inv, backend='numpy'), 1, sync=False) for _ in range(reps - 1)]))
            rows.append(dict(op='propagate', cloud=name, thinned=len(ids), points=len(xyz), masks=n_masks,
                             device_wall_ms=wall, numpy_wall_ms=numpy_wall))
            lines.append(f'{name:8s} {len(ids):8d} {len(xyz):8d} {n_masks:5d} {wall:11.1f} {numpy_wall:10.1f}')
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print(json.dumps(rows))


if __name__ == '__main__':
    main()
