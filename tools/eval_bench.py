"""Per-scan cost of the evaluators on synthetic sets: PanopticEval on a KITTI-like set (8 scans x 120 k
points, 19 classes, ~60 instances per scan) and semantic mIoU + accuracy + offset MAE on a
ScanNet-like set (4 scans x 150 k points, 20 classes), device path against numpy path.  The device
figure is split into the host-to-device copy of the inputs and the rest (kernels + read-back), each
the median over --reps runs.

    python tools/eval_bench.py [--reps 5]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import pointwise_cases as pc  # noqa: E402
from softgroup_amd.evaluation import (PanopticEval, evaluate_offset_mae, evaluate_semantic_acc,  # noqa: E402
                                      evaluate_semantic_miou)

THING = ['car', 'bicycle', 'motorcycle', 'truck', 'other-vehicle', 'person', 'bicyclist', 'motorcyclist']
STUFF = ['road', 'parking', 'sidewalk', 'other-ground', 'building', 'fence', 'vegetation', 'trunk', 'terrain',
         'pole', 'traffic-sign']


def timed(fn, reps, sync=True):
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


def h2d(arrays):
    for a in arrays:
        t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a)
        t.to('cuda')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    warnings.simplefilter('ignore', RuntimeWarning)
    out = {}

    preds, sems, insts = [list(x) for x in zip(*[pc.kitti_like(100 + s, 120000) for s in range(8)])]
    n_scans = len(preds)
    quiet = open(os.devnull, 'w')

    def pan(device):
        saved, sys.stdout = sys.stdout, quiet
        try:
            return PanopticEval(THING, STUFF, device=device).evaluate(preds, sems, insts)
        finally:
            sys.stdout = saved

    pan('cuda')                                                     # warm-up (library, allocator)
    dev = timed(lambda: pan('cuda'), args.reps)
    copy = timed(lambda: h2d(preds + sems + insts), args.reps)
    host = timed(lambda: pan('cpu'), max(1, args.reps // 2), sync=False)
    out['panoptic_kitti_like'] = dict(scans=n_scans, points_per_scan=120000,
                                      device_ms_per_scan=1e3 * dev / n_scans,
                                      device_h2d_ms_per_scan=1e3 * copy / n_scans,
                                      device_rest_ms_per_scan=1e3 * (dev - copy) / n_scans,
                                      numpy_ms_per_scan=1e3 * host / n_scans)

    sp, sg, op, og, inst = [list(x) for x in zip(*[pc.scannet_like(200 + s, 150000) for s in range(4)])]
    n_scans = len(sp)

    def sem(device):
        evaluate_semantic_miou(sp, sg, device=device)
        evaluate_semantic_acc(sp, sg, device=device)
        evaluate_offset_mae(op, og, inst, device=device)

    sem('cuda')
    dev = timed(lambda: sem('cuda'), args.reps)
    # the three calls copy pred + gt twice and offsets + instances once
    copy = timed(lambda: (h2d(sp + sg), h2d(sp + sg), h2d(op + og + inst)), args.reps)
    host = timed(lambda: sem('cpu'), max(1, args.reps // 2), sync=False)
    out['semantic_scannet_like'] = dict(scans=n_scans, points_per_scan=150000,
                                        device_ms_per_scan=1e3 * dev / n_scans,
                                        device_h2d_ms_per_scan=1e3 * copy / n_scans,
                                        device_rest_ms_per_scan=1e3 * (dev - copy) / n_scans,
                                        numpy_ms_per_scan=1e3 * host / n_scans)
    for k, v in out.items():
        print(k, ' '.join(f'{kk}={vv:.3f}' if isinstance(vv, float) else f'{kk}={vv}' for kk, vv in v.items()))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
