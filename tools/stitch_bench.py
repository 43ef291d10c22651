"""Cost of tiling a large cloud and of stitching the tiles' instances (softgroup_amd.data.tile_cloud,
softgroup_amd.util.stitch_results) on a scene_s2-style cloud of about 2.4 M points (a 24 x 20 m room shell with 12
boxes) cut into 4 x 4 square tiles of 6.25 m with a 0.5 m margin.

Two instance sets: about 100 and about 300 synthetic instances per tile (the points of the cells of a coarse
grid, so that instances straddle every cut); the per-tile "scan" reports for every such instance exactly its points
in the tile, as RLE dicts.

Timed, each the median of --reps runs after a warm-up, all in one run:
  tile_cloud        device_kernel_ms  sg_tile_assign_count + _fill on a resident cloud, from HIP events (the
                                      read-back of (T, total) between them included)
                    device_wall_ms    tile_cloud(CUDA xyz, backend='device'), wall time to a synchronise
                    numpy_wall_ms     tile_cloud(numpy xyz, backend='numpy')
  stitch_results    device_wall_ms / numpy_wall_ms of the whole call (RLE dicts in, RLE dicts out) and
                    device_event_ms of the same device call between two events
The device and numpy results are compared for equality before anything is timed.

    python tools/stitch_bench.py [--reps 5] [--out profiles/stitch_bench.txt]
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
from softgroup_amd.data import tile_cloud  # noqa: E402
from softgroup_amd.util import stitch_results  # noqa: E402
from softgroup_amd.util.rle import rle_encode_runs  # noqa: E402

SIZE, MARGIN, ORIGIN = 6.25, 0.5, (-0.5, -0.5)
BLOBS = {100: 0.72, 300: 0.39}          # instances per tile -> side of the coarse cells (m)


def median_ms(fn, reps, events=False, warm=True):
    if warm:
        fn()
    wall, dev = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(e0.elapsed_time(e1))
    return (float(np.median(wall)), float(np.median(dev))) if events else float(np.median(wall))


def tile_scans(xyz, tiles, side):
    """one result dict per tile: every coarse cell with a point in the tile is an instance"""
    cell = np.floor(xyz[:, :2].astype(np.float64) / side).astype(np.int64)
    blob = (cell[:, 1] - cell[:, 1].min()) * (cell[:, 0].max() - cell[:, 0].min() + 1) + (cell[:, 0] - cell[:, 0].min())
    results = []
    for t, ids in enumerate(tiles.point_ids):
        local = blob[ids]
        order = np.argsort(local, kind='stable')
        cut = np.flatnonzero(np.diff(local[order])) + 1
        insts = []
        for grp in np.split(order, cut):
            grp = np.sort(grp)
            head = np.concatenate([[True], np.diff(grp) > 1])
            starts = grp[head]
            ends = grp[np.concatenate([head[1:], [True]])] + 1
            b = int(local[grp[0]])
            insts.append(dict(scan_id='bench', label_id=1 + b % 3, conf=0.2 + 1e-5 * b + 1e-7 * t,
                              pred_mask=rle_encode_runs(ids.size, starts, ends - starts)))
        results.append(dict(scan_id='bench', semantic_preds=(local % 20).astype(np.int64), pred_instances=insts))
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--n', type=int, default=2400000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'stitch_bench.txt'))
    args = ap.parse_args()
    xyz, _, _ = synthetic.scene_s2(seed=1, n=args.n, room_scale=4.0)
    xyz = np.ascontiguousarray(xyz, np.float32)
    d_xyz = torch.from_numpy(xyz).cuda()
    lines = [f'device {torch.cuda.get_device_name(0)}; {xyz.shape[0]} points, tiles {SIZE} m, margin {MARGIN} m; '
             f'ms, medians of {args.reps} after a warm-up']

    tiles = tile_cloud(xyz, size=SIZE, margin=MARGIN, origin=ORIGIN, backend='numpy')
    d_tiles = tile_cloud(d_xyz, size=SIZE, margin=MARGIN, origin=ORIGIN, backend='device')
    for name in ('cells', 'tile_off', 'tile_points', 'core_tile', 'core_pos'):
        assert np.array_equal(np.asarray(getattr(tiles, name)), getattr(d_tiles, name).cpu().numpy()), name
    dev_wall, dev_kernel = median_ms(lambda: tile_cloud(d_xyz, size=SIZE, margin=MARGIN, origin=ORIGIN, backend='device'),
                                     args.reps, events=True)
    np_wall = median_ms(lambda: tile_cloud(xyz, size=SIZE, margin=MARGIN, origin=ORIGIN, backend='numpy'), args.reps)
    row = dict(op='tile_cloud', tiles=len(tiles), entries=int(tiles.offsets[-1]), device_kernel_ms=round(dev_kernel, 3),
               device_wall_ms=round(dev_wall, 3), numpy_wall_ms=round(np_wall, 3))
    lines.append(json.dumps(row))
    print(lines[-1], flush=True)

    for per_tile, side in BLOBS.items():
        results = tile_scans(xyz, tiles, side)
        n_inst = sum(len(r['pred_instances']) for r in results)
        a = stitch_results(results, tiles, backend='device')
        b = stitch_results(results, tiles, backend='numpy')
        assert [(i['label_id'], i['conf'], i['pred_mask']) for i in a['pred_instances']] == \
            [(i['label_id'], i['conf'], i['pred_mask']) for i in b['pred_instances']]
        assert np.array_equal(a['semantic_preds'], b['semantic_preds'])
        dev_wall, dev_event = median_ms(lambda: stitch_results(results, tiles, backend='device'), args.reps, events=True)
        np_wall = median_ms(lambda: stitch_results(results, tiles, backend='numpy'), args.reps, warm=False)      # (warm: the run above)
        row = dict(op='stitch_results', per_tile=round(n_inst / len(tiles)), tile_instances=n_inst,
                   objects=len(a['pred_instances']), device_event_ms=round(dev_event, 3),
                   device_wall_ms=round(dev_wall, 3), numpy_wall_ms=round(np_wall, 3))
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
