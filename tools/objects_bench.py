"""Cost of the object table (softgroup_amd.util.describe_instances / ops.objects) on synthetic instance lists: a
ScanNet-like cloud (150 k points, 100 and 300 masks) and an STPLS3D-like cloud (600 k points, 300 masks).  The cloud
is synthetic.scene_s2 and the masks are those of tools/split_bench.py (90 % of the points of one object plus 30 stray
points, every fifth mask two objects); RLE dicts, what forward_test returns.  yaw_steps 90, refine 0, colours and an
18-class semantic vote.

Reported per list, all in the same run, each the median over --reps runs after a warm-up (min .. max in brackets):
  moments_ms / extents_ms / hist_ms   the three C entries on bit rows and arrays already on the device, HIP events
  device_wall_ms    describe_instances(backend='device'): RLE text -> bits -> the entries -> one read-back, wall time
  numpy_wall_ms     describe_instances(backend='numpy'), the twins, wall time
  naive_ms          dense decode plus a per-mask numpy loop (coords[mask].min(0) and so on), ONE run
The two backends must return the same table, byte for byte, before anything is timed.

    python tools/objects_bench.py [--reps 5] [--out profiles/objects_bench.txt]
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
from softgroup_amd.ops import objects as OB  # noqa: E402
from softgroup_amd.util import describe_instances, rle_decode  # noqa: E402
from softgroup_amd.util import masks as UM  # noqa: E402
from softgroup_amd.util.rle import rle_encode  # noqa: E402

CASES = [('scannet', 150000, 1.0, 100), ('scannet', 150000, 1.0, 300), ('stpls3d', 600000, 2.0, 300)]
YAW_STEPS, N_CLASSES = 90, 18


def instance_list(seed, n_points, room_scale, n_masks):
    xyz, rgb, inst = synthetic.scene_s2(seed=seed, n=n_points, room_scale=room_scale)
    rng = np.random.default_rng(seed)
    n_obj = int(inst.max()) + 1
    insts = []
    for k in range(n_masks):
        objs = rng.choice(n_obj, size=2 if k % 5 == 4 else 1, replace=False)
        m = np.isin(inst, objs) & (rng.random(xyz.shape[0]) < 0.9)
        m[rng.integers(xyz.shape[0], size=30)] = True
        insts.append(dict(scan_id='s', label_id=int(1 + objs[0] % 18), conf=float(f'{rng.uniform():.4f}'),
                          pred_mask=rle_encode(m.astype(np.int64))))
    sem = (np.maximum(inst, 0) % N_CLASSES).astype(np.int64)
    return np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(rgb, np.float32), sem, insts


def naive(insts, xyz, rgb, sem):
    """what a consumer writes today: decode every mask, then numpy per mask"""
    theta, table = OB.yaw_table(YAW_STEPS)
    out = []
    for inst in insts:
        mask = rle_decode(inst['pred_mask']).astype(bool)
        p = xyz[mask].astype(np.float64)
        u = p[:, 0:1] * table[None, :, 0] + p[:, 1:2] * table[None, :, 1]
        v = p[:, 1:2] * table[None, :, 0] - p[:, 0:1] * table[None, :, 1]
        area = (u.max(0) - u.min(0)) * (v.max(0) - v.min(0))
        out.append((int(mask.sum()), p.min(0), p.max(0), p.mean(0), np.cov(p.T), rgb[mask].mean(0),
                    int(np.argmin(area)), np.bincount(sem[mask], minlength=N_CLASSES).argmax()))
    return out


def wall_ms(fn, reps, sync):
    ts = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return ts


def event_ms(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def cell(ts, digits=3):
    return f'{np.median(ts):.{digits}f} [{min(ts):.{digits}f} .. {max(ts):.{digits}f}]'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'objects_bench.txt'))
    args = ap.parse_args()
    dev = torch.device('cuda')
    lines = [f'# tools/objects_bench.py --reps {args.reps}  ({torch.cuda.get_device_name(0)}); ms, median '
             f'[min .. max]; yaw_steps {YAW_STEPS}, refine 0, colours, {N_CLASSES} classes; naive: one run',
             f'{"set":8s} {"points":>7s} {"masks":>5s} {"pairs":>9s} | moments | extents | hist | device_wall | '
             f'numpy_wall | naive']
    rows = []
    for c, (name, n_points, room_scale, n_masks) in enumerate(CASES):
        xyz, rgb, sem, insts = instance_list(20 + c, n_points, room_scale, n_masks)
        n_points = xyz.shape[0]
        kw = dict(colors=rgb, semantic=sem, n_classes=N_CLASSES, yaw_steps=YAW_STEPS)
        want = describe_instances(insts, xyz, backend='numpy', **kw)                      # (also the warm-up)
        got = describe_instances(insts, xyz, backend='device', **kw)
        assert sorted(got) == sorted(want)
        for key in want:
            assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), (name, key)
        device_wall = wall_ms(lambda: describe_instances(insts, xyz, backend='device', **kw), args.reps, True)
        numpy_wall = wall_ms(lambda: describe_instances(insts, xyz, backend='numpy', **kw), args.reps, False)
        naive_ms = wall_ms(lambda: naive(insts, xyz, rgb, sem), 1, False)
        packed = UM.packed_rows(insts, n_points)
        pairs = int(np.unpackbits(packed, axis=1, bitorder='little')[:, :n_points].sum())
        bits = torch.from_numpy(packed.view(np.int32).reshape(n_masks, -1)).to(dev)
        d_xyz, d_rgb, d_sem = (torch.from_numpy(a).to(dev) for a in (xyz, rgb, sem))
        table = torch.from_numpy(OB.yaw_table(YAW_STEPS)[1]).to(dev)
        entries = [lambda: OB.instance_moments(bits, n_points, d_xyz, d_rgb),
                   lambda: OB.instance_extents(bits, n_points, d_xyz, table),
                   lambda: OB.instance_class_hist(bits, n_points, d_sem, N_CLASSES)]
        timed = []
        for fn in entries:
            fn()
            timed.append(event_ms(fn, args.reps))
        rows.append(dict(set=name, points=n_points, masks=n_masks, pairs=pairs, moments_ms=timed[0],
                         extents_ms=timed[1], hist_ms=timed[2], device_wall_ms=device_wall, numpy_wall_ms=numpy_wall,
                         naive_ms=naive_ms))
        lines.append(f'{name:8s} {n_points:7d} {n_masks:5d} {pairs:9d} | {cell(timed[0])} | {cell(timed[1])} | '
                     f'{cell(timed[2])} | {cell(device_wall, 1)} | {cell(numpy_wall, 1)} | {naive_ms[0]:.0f}')
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print(json.dumps(rows))


if __name__ == '__main__':
    main()
