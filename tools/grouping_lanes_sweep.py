"""Lanes per node of the grouping head's list kernels (sg_grouping_set_lanes) against the mean list length:
the ball query and the clustering of one cloud with every forced width, results compared with the 64-lane
run, event times of the two operator calls.  Per-kernel times: run it under rocprofv3 --kernel-trace (the
kernel names carry the width).
Usage (GPU box): python tools/grouping_lanes_sweep.py <mean list length | g1> [points] [reps]
  a number: `points` uniform points in a cube sized for that mean at r = 0.04;  g1: bench.py's G1 cloud."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from softgroup_amd import _lib as L, ops, synthetic  # noqa: E402

R = 0.04


def events_ms(fn, reps):
    for _ in range(2):
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


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else '4'
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    if what == 'g1':
        xyz = synthetic.scene_g1(seed=2)
    else:
        side = (n * 4.0 / 3.0 * np.pi * R ** 3 / max(float(what) - 1.0, 1e-3)) ** (1.0 / 3.0)
        xyz = (np.random.default_rng(3).random((n, 3)) * side).astype(np.float32)
    pts = torch.from_numpy(np.ascontiguousarray(xyz)).cuda()
    n = pts.shape[0]
    bi = torch.zeros(n, dtype=torch.int32, device='cuda')
    bo = torch.tensor([0, n], dtype=torch.int32, device='cuda')
    mean = torch.tensor([-1.0])
    lib = L.lib()
    prev = lib.sg_grouping_set_lanes(64)
    try:
        want = None
        for lanes in (64, 32, 16, 8, 0):
            lib.sg_grouping_set_lanes(lanes)
            with torch.no_grad():
                idx, sl = ops.ballquery_batch_p(pts, bi, bo, R, 300)
                ci, co = ops.bfs_cluster(mean, idx, sl, 100.0, 0)
                got = [t.cpu() for t in (idx, sl, ci, co)]
                if want is None:
                    want = got
                same = all(torch.equal(a, b) for a, b in zip(got, want))
                t_bq = events_ms(lambda: ops.ballquery_batch_p(pts, bi, bo, R, 300), reps)
                t_bfs = events_ms(lambda: ops.bfs_cluster(mean, idx, sl, 100.0, 0), reps)
            print(f'{what}: n {n} mean list {idx.numel() / n:.1f} lanes {lanes:2d}: ball_query {t_bq:.3f} ms '
                  f'bfs_cluster {t_bfs:.3f} ms  clusters {co.numel() - 1}  identical to 64 lanes: {same}')
    finally:
        lib.sg_grouping_set_lanes(prev)


if __name__ == '__main__':
    main()
