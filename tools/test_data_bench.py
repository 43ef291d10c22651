"""Times the test-time data transform (softgroup_amd.data.TestTransform) against ``scan_item`` on the same host and
prints one JSON line per scan, then one for the test loop:

  * scannet (150k points / 40 instances), kitti (120k points from raw 32-bit label words, rank relabel),
    s3dis_x4 (1M points, x4_split), stpls3d (600k points / 300 instances);
  * per scan: ``h2d_ms`` (host arrays to device tensors), ``item_ms`` (the device item from resident inputs),
    split by a kernel trace into ``kernels_ms`` (GPU time of the item's kernels and device copies) and
    ``readback_ms`` (its device-to-host copies; the rest of item_ms is host work and launch), ``batch_ms``
    (item from host arrays + collate, voxel index included), ``scan_item_ms`` (numpy, this host);
  * loop: ``prefetch_device`` with the transform as its collate on two loader threads, ``forward_test`` on the
    consumer, fed from host arrays: scans/s.

Usage: python tools/test_data_bench.py [--reps 10] [--cpu-reps 2] [--loop-scans 24]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from softgroup_amd import data, synthetic  # noqa: E402
from softgroup_amd.data import TestTransform  # noqa: E402
from test_test_data import blobs, kitti_words, kitti_yaml_map, labelled, voxel_cfg  # noqa: E402


def scans():
    xyz, rgb, inst = blobs(150000, 40, 1)
    yield 'scannet', dict(dataset='scannetv2'), dict(xyz=xyz, rgb=rgb, **_labels(labelled(inst, 2)))
    xyz, rem, words = kitti_words()
    yield 'kitti', dict(dataset='kitti', learning_map=kitti_yaml_map()), dict(xyz=xyz, rgb=rem, label_words=words)
    xyz, rgb, inst = blobs(1000000, 40, 4, extent=(10.0, 8.0, 3.0))
    yield 's3dis_x4', dict(dataset='s3dis', x4_split=True), dict(xyz=xyz, rgb=rgb, **_labels(labelled(inst, 0, 13)))
    xyz, rgb, inst = blobs(600000, 300, 2, extent=(50.0, 50.0, 10.0))
    yield 'stpls3d', dict(dataset='stpls3d'), dict(xyz=xyz, rgb=rgb, **_labels(labelled(inst, 1, 14)))


def _labels(sl):
    return dict(semantic_label=sl[0], instance_label=sl[1])


def timed(fn, reps, sync=True):
    fn()
    if sync:
        torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    if sync:
        torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def trace_split(fn):
    """GPU time of fn's kernels / device copies and of its device-to-host copies (ms), from a kernel trace"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    kern = d2h = 0.0
    for e in prof.events():
        if getattr(e, 'device_type', None) is None or str(e.device_type).endswith('CPU'):
            continue
        us = e.device_time if hasattr(e, 'device_time') else e.cuda_time
        name = e.name.lower()
        if 'dtoh' in name or 'devicetohost' in name or 'd2h' in name:
            d2h += us
        else:
            kern += us
    return kern / 1e3, d2h / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--cpu-reps', type=int, default=2)
    ap.add_argument('--loop-scans', type=int, default=24)
    a = ap.parse_args()
    for name, tkw, call in scans():
        dev = TestTransform(voxel_cfg(tkw['dataset']), **tkw)
        cpu = TestTransform(voxel_cfg(tkw['dataset']), device='cpu', **tkw)
        resident = {k: torch.as_tensor(v).cuda() for k, v in call.items()}
        res = {'scan': name, 'points': int(call['xyz'].shape[0])}
        res['h2d_ms'] = timed(lambda: [torch.as_tensor(v).cuda() for v in call.values()], a.reps)
        item = lambda: dev(**resident)     # noqa: E731
        res['item_ms'] = timed(item, a.reps)
        try:
            res['kernels_ms'], res['readback_ms'] = trace_split(item)
        except Exception as e:  # noqa: BLE001 -- the trace is optional
            res['trace_error'] = repr(e)[:120]
        res['item_from_host_ms'] = timed(lambda: dev(**call), a.reps)
        res['batch_ms'] = timed(lambda: dev.collate([call]), a.reps)
        res['scan_item_ms'] = timed(lambda: cpu(**call), a.cpu_reps, sync=False)
        res['speedup_vs_scan_item'] = res['scan_item_ms'] / res['batch_ms']
        print(json.dumps({k: round(v, 3) if isinstance(v, float) else v for k, v in res.items()}), flush=True)

    # the test loop: prefetch_device(transform as collate) -> forward_test, from host arrays
    tf = TestTransform(voxel_cfg('scannetv2'))
    pool = []
    for s in range(4):
        xyz, rgb, inst = synthetic.scene_s2(seed=s)
        pool.append((xyz, rgb) + labelled(inst, 2) + (f'scan{s}', ))
    model = synthetic.build_model(seed=0)
    model.async_results = False
    batches = lambda k: ([pool[i % len(pool)]] for i in range(k))     # noqa: E731
    with torch.no_grad():
        for b in data.prefetch_device(batches(4), collate=tf.collate, workers=2):
            model(b)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for b in data.prefetch_device(batches(a.loop_scans), collate=tf.collate, workers=2):
            model(b)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
    print(json.dumps({'loop': 'prefetch_device + TestTransform + forward_test', 'points': 150000,
                      'scans': a.loop_scans, 'scans_per_s': round(a.loop_scans / dt, 2),
                      'ms_per_scan': round(dt / a.loop_scans * 1e3, 3)}), flush=True)


if __name__ == '__main__':
    main()
