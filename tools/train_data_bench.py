"""Times the training-time data transform (softgroup_amd.data.TrainTransform) on one 150k-point ScanNet-like
scan (synthetic.scene_s2, the ScanNet voxel config) and prints one JSON line:

  * device_ms_per_scan / numpy_rng_ms_per_scan: TrainTransform on the GPU with rng='device' / rng='numpy'
    (inputs already resident, as a loader that keeps them there would have them);
  * device_ms_per_batch4: four scans + collate_train_device (voxel index included), rng='device';
  * cpu_ms_per_scan: the numpy restatement (device='cpu', rng='numpy'), single process.

Usage: python tools/train_data_bench.py [--reps 10] [--cpu-reps 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from softgroup_amd import synthetic  # noqa: E402
from softgroup_amd.data import TrainTransform, collate_train_device  # noqa: E402

CFG = dict(scale=50, spatial_shape=[128, 512], max_npoint=250000, min_npoint=5000)


def scan(seed):
    xyz, rgb, inst = synthetic.scene_s2(seed=seed)
    sem = np.where(inst >= 0, 2 + inst % 18, 0).astype(np.float64)
    return xyz, rgb, sem, inst.astype(np.float64)


def timed(fn, reps, sync):
    fn()
    if sync:
        torch.cuda.synchronize()
    t = time.perf_counter()
    for i in range(reps):
        fn(i)
    if sync:
        torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--cpu-reps', type=int, default=2)
    a = ap.parse_args()
    host = [scan(s) for s in (1, 2, 3, 4)]
    dev = [tuple(torch.as_tensor(v).cuda() for v in s) for s in host]
    fast = TrainTransform(CFG, rng='device', seed=0)
    slow = TrainTransform(CFG, rng='numpy')
    cpu = TrainTransform(CFG, rng='numpy', device='cpu')
    np.random.seed(0)
    torch.manual_seed(0)
    res = {
        'device_ms_per_scan': timed(lambda i=0: fast(*dev[0], index=i), a.reps, True),
        'numpy_rng_ms_per_scan': timed(lambda i=0: slow(*dev[0], index=i), a.reps, True),
        'device_ms_per_batch4': timed(lambda i=0: collate_train_device(
            [fast(*s, index=4 * i + j) for j, s in enumerate(dev)]), a.reps, True),
        'device_host_inputs_ms_per_scan': timed(lambda i=0: fast(*host[0], index=i), a.reps, True),
        'cpu_ms_per_scan': timed(lambda i=0: cpu(*host[0], index=i), a.cpu_reps, False),
        'points': int(host[0][0].shape[0]),
    }
    print(json.dumps({k: round(v, 3) if isinstance(v, float) else v for k, v in res.items()}))


if __name__ == '__main__':
    main()
