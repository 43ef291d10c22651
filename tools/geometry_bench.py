"""Cost of making superpoints (softgroup_amd.ops.geometry: knn, point_normals, grow_segments; util.make_superpoints)
on synthetic.scene_s2 clouds of 150 k and 600 k points with k = 8 / 16 / 32.

Before anything is timed the device is compared with the twins: knn byte for byte with ``knn_numpy`` on the first
--check points of the cloud (the brute force is O(N x N): infeasible on the whole cloud, as for nearest_index) and, on
the whole cloud, its distances with scipy's cKDTree (sorted d2 within 1e-12 relative; the tree is not tie-exact, so
indices are not compared); the growth byte for byte with ``grow_segments_numpy`` on the whole cloud (the twin's
normals on both sides); the normals by their worst angle to ``point_normals_numpy`` (reported, and held to 1e-6 rad
where the twin's relative eigen-gap is at least 1e-3).

Reported per cloud and k, all in the same run, each the median over --reps runs after a warm-up (ms):
  knn            ops.knn on a cloud already on the device with the default cell, from HIP events (read-back included)
  knn_wall       the same call by wall clock
  ckdtree        scipy.spatial.cKDTree(xyz).query(xyz, k + 1, workers=-1), build + query, wall clock -- NOT tie-exact
  normals        ops.point_normals on the device, from HIP events;  normals_numpy: the twin, wall clock
  grow           ops.grow_segments on the device, from HIP events;   grow_numpy: the twin, wall clock
  make_sp        util.make_superpoints on the device cloud, wall clock (all three and their read-backs)
  scanned        queries the full scan answered;  segs: segments of make_superpoints with its defaults

    python tools/geometry_bench.py [--reps 5] [--check 20000] [--out profiles/geometry_bench.txt]
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
from softgroup_amd import synthetic  # noqa: E402
from softgroup_amd.ops import geometry as G  # noqa: E402
from softgroup_amd.util import make_superpoints  # noqa: E402

try:
    from scipy.spatial import cKDTree
except ImportError:                                         # the column then reads nan
    cKDTree = None

CASES = [('scannet', 150000, 1.0), ('stpls3d', 600000, 2.0)]
KS = (8, 16, 32)


def wall_ms(fn, reps, sync=True):
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


def event_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int64), b[1].view(np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--check', type=int, default=20000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'geometry_bench.txt'))
    args = ap.parse_args()
    dev = torch.device('cuda')
    head = ('set', 'points', 'k', 'knn', 'knn_wall', 'ckdtree', 'normals', 'normals_numpy', 'grow', 'grow_numpy',
            'make_sp', 'scanned', 'segs', 'worst_angle')
    lines = [f'# tools/geometry_bench.py --reps {args.reps}  ({torch.cuda.get_device_name(0)}); ms, median; ckdtree is '
             'not tie-exact (distances compared, indices not)',
             ' '.join(f'{h:>{max(len(h), 9)}s}' for h in head)]
    rows = []
    for c, (name, n_points, room_scale) in enumerate(CASES):
        xyz = synthetic.scene_s2(seed=30 + c, n=n_points, room_scale=room_scale)[0].astype(np.float32)
        n_points = xyz.shape[0]
        d_xyz = torch.from_numpy(xyz).to(dev)
        for k in KS:
            # ---- equality first (also the warm-up)
            part = xyz[:args.check]
            assert same_bits(G.knn(part, k, backend='device'), G.knn_numpy(part, k)), (name, k)
            d_idx, d_d2, scanned = G.knn(d_xyz, k, return_meta=True)
            idx, d2 = d_idx.cpu().numpy(), d_d2.cpu().numpy()
            if cKDTree is not None:
                dist = cKDTree(xyz).query(xyz, k + 1, workers=-1)[0][:, 1:].astype(np.float64)
                assert np.allclose(dist * dist, d2, rtol=1e-12, atol=0.0), (name, k)
            h_nm, h_curv = G.point_normals_numpy(xyz, idx)
            d_nm, d_curv = G.point_normals(d_xyz, d_idx)
            lam = G._normals_f64(xyz, idx.astype(np.int64), 3, return_eigenvalues=True)[2]
            a, b = d_nm.cpu().numpy().astype(np.float64), h_nm.astype(np.float64)
            angle = np.arcsin(np.minimum(np.linalg.norm(np.cross(a, b), axis=1), 1.0))
            with np.errstate(invalid='ignore', divide='ignore'):
                judged = (lam[:, 1] - lam[:, 0]) / lam[:, 2] >= 1e-3
            worst = float(angle[judged].max())
            assert worst <= 1e-6 and np.array_equal((a == 0).all(1), (b == 0).all(1)), (name, k, worst)
            t_nm, t_curv = torch.from_numpy(h_nm).to(dev), torch.from_numpy(h_curv).to(dev)
            h_sp = G.grow_segments_numpy(idx, h_nm, h_curv, d2)
            d_sp = G.grow_segments(d_idx, t_nm, t_curv, d_d2)
            assert h_sp[1] == d_sp[1] and np.array_equal(h_sp[0], d_sp[0].cpu().numpy()), (name, k)
            segs = int(make_superpoints(d_xyz, k=k).max().item()) + 1
            # ---- times
            row = dict(set=name, points=n_points, k=k, scanned=scanned, segs=segs, worst_angle=worst)
            row['knn'] = event_ms(lambda: G.knn(d_xyz, k), args.reps)
            row['knn_wall'] = wall_ms(lambda: G.knn(d_xyz, k), args.reps)
            row['ckdtree'] = float('nan') if cKDTree is None else wall_ms(
                lambda: cKDTree(xyz).query(xyz, k + 1, workers=-1), args.reps, sync=False)
            row['normals'] = event_ms(lambda: G.point_normals(d_xyz, d_idx), args.reps)
            row['normals_numpy'] = wall_ms(lambda: G.point_normals_numpy(xyz, idx), args.reps, sync=False)
            row['grow'] = event_ms(lambda: G.grow_segments(d_idx, t_nm, t_curv, d_d2), args.reps)
            row['grow_numpy'] = wall_ms(lambda: G.grow_segments_numpy(idx, h_nm, h_curv, d2), args.reps, sync=False)
            row['make_sp'] = wall_ms(lambda: make_superpoints(d_xyz, k=k), args.reps)
            rows.append(row)
            cells = [f'{row[h]:>{max(len(h), 9)}.3g}' if h == 'worst_angle' else
                     f'{row[h]:>{max(len(h), 9)}.3f}' if isinstance(row[h], float) else f'{row[h]!s:>{max(len(h), 9)}s}'
                     for h in head]
            lines.append(' '.join(cells))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print(json.dumps(rows))


if __name__ == '__main__':
    main()
