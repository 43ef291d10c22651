"""Cost of greedy mask NMS (softgroup_amd.util.nms_instances / ops.mask_nms) on synthetic instance lists:
a ScanNet-like set (150 k points, 100 and 300 masks) and an STPLS3D-like set (600 k points, 300 and 1000 masks).
Masks are noisy copies of n / 3 objects laid out in chunks of consecutive points, as RLE dicts (what
forward_test returns), %.4f confidences, 3 classes; thr 0.5, 'iou', class-aware.

Reported per list, all in the same run, each the median over --reps runs:
  device_kernel_ms   sg_mask_nms alone on bit rows already on the device, from HIP events
  device_wall_ms     nms_instances(backend='device'): RLE text -> sg_inst_rle_parse -> bits -> sg_mask_nms ->
                     keep flags on the host, wall time
  numpy_wall_ms      nms_instances(backend='numpy'): RLE -> packed rows -> popcounts, wall time
  numpy_kernel_ms    mask_nms_numpy alone on packed rows already built
  naive_wall_ms      what users do today: every RLE string decoded to a dense bool row, then the Python double
                     loop over (kept, later) pairs with (a & b).sum(); one run, lists of at most --naive-max masks
All paths must keep the same instances.

    python tools/mask_nms_bench.py [--reps 5] [--out profiles/mask_nms_bench.txt]
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
from softgroup_amd.ops import nms as MN  # noqa: E402
from softgroup_amd.util import nms_instances  # noqa: E402
from softgroup_amd.util.rle import rle_decode, rle_encode  # noqa: E402

CASES = [('scannet', 150000, 100), ('scannet', 150000, 300), ('stpls3d', 600000, 300), ('stpls3d', 600000, 1000)]
THR = 0.5


def instance_list(seed, n_points, n_masks, chunk=500):
    rng = np.random.default_rng(seed)
    n_chunks = n_points // chunk
    n_obj = max(2, n_masks // 3)
    owner = rng.integers(0, 2 * n_obj, n_chunks)                 # half of the chunks are background
    cls = rng.integers(1, 4, n_obj)
    insts = []
    for _ in range(n_masks):
        g = rng.integers(0, n_obj)
        m = np.repeat((owner == g) & (rng.uniform(size=n_chunks) < rng.uniform(0.5, 0.95)), chunk)
        full = np.zeros(n_points, dtype=np.int64)
        full[:m.size] = m
        insts.append(dict(scan_id='s', label_id=int(cls[g]), conf=float(f'{rng.uniform():.4f}'),
                          pred_mask=rle_encode(full)))
    return insts


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


def naive(insts, thr):
    masks = [rle_decode(i['pred_mask']).astype(bool) for i in insts]
    order = sorted(range(len(insts)), key=lambda k: (-insts[k]['conf'], k))
    kept = []
    for k in order:
        a = masks[k]
        for j in kept:
            if insts[j]['label_id'] != insts[k]['label_id']:
                continue
            inter = int((a & masks[j]).sum())
            union = int(a.sum()) + int(masks[j].sum()) - inter
            if union and inter / union > thr:
                break
        else:
            kept.append(k)
    return sorted(kept)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--naive-max', type=int, default=300)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mask_nms_bench.txt'))
    args = ap.parse_args()
    dev = torch.device('cuda')
    lines = [f'# tools/mask_nms_bench.py --reps {args.reps}  ({torch.cuda.get_device_name(0)}); ms, median; '
             f"thr {THR}, 'iou', class-aware",
             f'{"set":8s} {"points":>7s} {"masks":>5s} {"kept":>5s} {"device_kernel":>13s} {"device_wall":>11s} '
             f'{"numpy_kernel":>12s} {"numpy_wall":>10s} {"naive_wall":>10s}']
    rows = []
    for c, (name, n_points, n_masks) in enumerate(CASES):
        insts = instance_list(10 + c, n_points, n_masks)
        ids = {id(x): k for k, x in enumerate(insts)}
        want = [ids[id(x)] for x in nms_instances(insts, THR, backend='numpy')]
        got = [ids[id(x)] for x in nms_instances(insts, THR, backend='device')]          # (also the warm-up)
        assert got == want, (name, n_masks)
        device_wall = median_s(lambda: nms_instances(insts, THR, backend='device'), args.reps)
        numpy_wall = median_s(lambda: nms_instances(insts, THR, backend='numpy'), max(1, args.reps // 2), sync=False)
        from softgroup_amd.util import masks as UM
        packed = UM.packed_rows(insts, n_points)
        scores = np.array([i['conf'] for i in insts], np.float32)
        labels = np.array([i['label_id'] for i in insts], np.int32)
        numpy_kernel = median_s(lambda: MN.mask_nms_numpy(packed, n_points, scores, labels, THR),
                                max(1, args.reps // 2), sync=False)
        bits = torch.from_numpy(packed.view(np.int32)).to(dev)
        d_s, d_l = torch.from_numpy(scores).to(dev), torch.from_numpy(labels).to(dev)
        keep, _ = MN.mask_nms(bits, n_points, d_s, d_l, THR)
        assert np.flatnonzero(keep.cpu().numpy()).tolist() == want
        ev = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            MN.mask_nms(bits, n_points, d_s, d_l, THR)
            b.record()
            torch.cuda.synchronize()
            ev.append(a.elapsed_time(b))
        device_kernel = float(np.median(ev))
        naive_wall = None
        if n_masks <= args.naive_max:
            t0 = time.perf_counter()
            kept = naive(insts, THR)
            naive_wall = time.perf_counter() - t0
            assert kept == want, (name, n_masks, 'naive')
        row = dict(set=name, points=n_points, masks=n_masks, kept=len(want), device_kernel_ms=device_kernel,
                   device_wall_ms=1e3 * device_wall, numpy_kernel_ms=1e3 * numpy_kernel, numpy_wall_ms=1e3 * numpy_wall,
                   naive_wall_ms=None if naive_wall is None else 1e3 * naive_wall)
        rows.append(row)
        lines.append(f'{name:8s} {n_points:7d} {n_masks:5d} {len(want):5d} {device_kernel:13.3f} '
                     f'{1e3 * device_wall:11.1f} {1e3 * numpy_kernel:12.1f} {1e3 * numpy_wall:10.1f} '
                     + (f'{1e3 * naive_wall:10.1f}' if naive_wall is not None else f'{"not run":>10s}'))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print(json.dumps(rows))


if __name__ == '__main__':
    main()
