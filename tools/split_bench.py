"""Cost of cutting instance masks into connected components (softgroup_amd.util.split_instances /
ops.mask_components) on synthetic instance lists: a ScanNet-like cloud (150 k points, 100 and 300 masks) and an
STPLS3D-like cloud (600 k points, 300 masks).  The cloud is synthetic.scene_s2 (a room shell and 12 box-shaped
objects at ~900 points / m^2); a mask is 90 % of the points of one object plus 30 stray points anywhere, every fifth
mask two objects welded together; RLE dicts, what forward_test returns.  radius 0.05, min_npoint 50, 'split'.

Reported per list, all in the same run, each the median over --reps runs after a warm-up:
  device_kernel_ms   sg_mask_split_count + _fill on bit rows and coordinates already on the device, from HIP events
                     (the read-back of meta between the passes included)
  device_wall_ms     split_instances(backend='device'): RLE text -> bits -> components -> runs -> RLE text, wall time
  numpy_wall_ms      split_instances(backend='numpy'), wall time
The two backends must return the same list, byte for byte, before anything is timed.

    python tools/split_bench.py [--reps 5] [--out profiles/split_bench.txt] [--sets scannet,stpls3d] [--append]

(the numpy path takes minutes on the large list: --sets and --append let the table be written in several runs)
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
from softgroup_amd.ops import split as MS  # noqa: E402
from softgroup_amd.util import masks as UM  # noqa: E402
from softgroup_amd.util import split_instances  # noqa: E402
from softgroup_amd.util.rle import rle_encode  # noqa: E402

CASES = [('scannet', 150000, 1.0, 100), ('scannet', 150000, 1.0, 300), ('stpls3d', 600000, 2.0, 300)]
RADIUS, MIN_NPOINT, MODE = 0.05, 50, 'split'


def instance_list(seed, n_points, room_scale, n_masks):
    xyz, _, inst = synthetic.scene_s2(seed=seed, n=n_points, room_scale=room_scale)
    rng = np.random.default_rng(seed)
    n_obj = int(inst.max()) + 1
    insts = []
    for k in range(n_masks):
        objs = rng.choice(n_obj, size=2 if k % 5 == 4 else 1, replace=False)
        m = np.isin(inst, objs) & (rng.random(xyz.shape[0]) < 0.9)
        m[rng.integers(xyz.shape[0], size=30)] = True
        insts.append(dict(scan_id='s', label_id=int(1 + objs[0] % 18), conf=float(f'{rng.uniform():.4f}'),
                          pred_mask=rle_encode(m.astype(np.int64))))
    return xyz, insts


def median_s(fn, reps, sync=True):
    ts = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def same(a, b):
    return len(a) == len(b) and all(x == y for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'split_bench.txt'))
    ap.add_argument('--sets', default='scannet,stpls3d')
    ap.add_argument('--append', action='store_true', help='add rows to --out instead of starting it')
    args = ap.parse_args()
    dev = torch.device('cuda')
    lines = [f'# tools/split_bench.py --reps {args.reps}  ({torch.cuda.get_device_name(0)}); ms, median; '
             f"radius {RADIUS}, min_npoint {MIN_NPOINT}, '{MODE}'",
             f'{"set":8s} {"points":>7s} {"masks":>5s} {"pairs":>9s} {"out":>5s} {"device_kernel":>13s} '
             f'{"device_wall":>11s} {"numpy_wall":>10s}']
    if args.append:
        lines = []
    rows = []
    for c, (name, n_points, room_scale, n_masks) in enumerate(CASES):
        if name not in args.sets.split(','):
            continue
        xyz, insts = instance_list(20 + c, n_points, room_scale, n_masks)
        par = (RADIUS, MIN_NPOINT, MODE)
        want = split_instances(insts, xyz, *par, backend='numpy')                       # (also the warm-up)
        got = split_instances(insts, xyz, *par, backend='device')
        assert same(got, want), (name, n_masks)
        assert len(want) > n_masks, 'the list must have masks to cut'
        d_xyz = torch.from_numpy(xyz).to(dev)
        device_wall = median_s(lambda: split_instances(insts, d_xyz, *par, backend='device'), args.reps)
        def numpy_run():
            split_instances(insts, xyz, *par, backend='numpy')
            print('.', end='', file=sys.stderr, flush=True)

        numpy_wall = median_s(numpy_run, args.reps, sync=False)
        packed = UM.packed_rows(insts, n_points)
        pairs = int(np.unpackbits(packed, axis=1, bitorder='little')[:, :n_points].sum())
        bits = torch.from_numpy(packed.view(np.int32)).to(dev)
        out = MS.mask_components(bits, n_points, d_xyz, *par)
        assert out[0].size(0) == len(want) and int(out[2].sum()) == sum(
            sum(int(t) for t in w['pred_mask']['counts'].split()[1::2]) for w in want)
        ev = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            MS.mask_components(bits, n_points, d_xyz, *par)
            b.record()
            torch.cuda.synchronize()
            ev.append(a.elapsed_time(b))
        device_kernel = float(np.median(ev))
        rows.append(dict(set=name, points=n_points, masks=n_masks, pairs=pairs, out=len(want),
                         device_kernel_ms=device_kernel, device_wall_ms=1e3 * device_wall,
                         numpy_wall_ms=1e3 * numpy_wall))
        lines.append(f'{name:8s} {n_points:7d} {n_masks:5d} {pairs:9d} {len(want):5d} {device_kernel:13.3f} '
                     f'{1e3 * device_wall:11.1f} {1e3 * numpy_wall:10.1f}')
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a' if args.append else 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print(json.dumps(rows))


if __name__ == '__main__':
    main()
