"""Cost of writing a test run's result files (softgroup_amd.util.results) for three synthetic scans:

  scannet  150 000 points (synthetic.scene_s2), 100 predicted masks + the ground-truth instance ids
  stpls3d  600 000 points (synthetic.scene_s2), 300 predicted masks + the ground-truth instance ids
  kitti    120 000 points (synthetic.scene_lidar), the panoptic words

Per scan, medians over --reps runs after a warm-up run:
  kernel_ms       device formatting, kernels only (HIP events around the launches)
  kernel_copy_ms  the same plus the copy of the text to pinned memory (events)
  device_wall_ms  save_* with backend='device', call to return: every file written and closed
  numpy_wall_ms   the same with backend='numpy'
  read_masks_*_ms load_pred_instances of the scan's masks, backend='device' and backend='numpy'
  read_ids_*_ms   read_int_lines of the scan's ground-truth ids, both backends (panoptic scan: no text to read)
The previous run's files are removed outside the timed region.  For the scannet scan the reference's method --
a dense mask from the run-length string and np.savetxt(fmt='%d') per mask -- is timed mask by mask on
--ref-masks masks after one warm-up mask; the median per mask times the number of masks is reported.

    python tools/save_results_bench.py [--reps 5] [--out DIR]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from softgroup_amd import _lib as L  # noqa: E402
from softgroup_amd import synthetic  # noqa: E402
from softgroup_amd.util import results as R  # noqa: E402
from softgroup_amd.util.rle import rle_decode, rle_encode  # noqa: E402

NYU_ID = (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39)
LEARNING_MAP_INV = {0: 0, 1: 10, 2: 11, 3: 15, 4: 18, 5: 20, 6: 30, 7: 31, 8: 32, 9: 40, 10: 44, 11: 48, 12: 49,
                    13: 50, 14: 51, 15: 70, 16: 71, 17: 72, 18: 80, 19: 81}


def instance_scan(name, seed, n, n_masks, chunk=200):
    """predicted masks = an object's points with chunks of consecutive points removed (mesh vertex order keeps
    an object's points in few runs), as the run-length dicts forward_test returns; ids as get_gt_instances'"""
    _, _, inst = synthetic.scene_s2(seed=seed, n=n)
    n = len(inst)
    rng = np.random.default_rng(seed)
    objects = np.unique(inst[inst >= 0])
    insts = []
    for k in range(n_masks):
        drop = np.repeat(rng.uniform(size=n // chunk + 1) < 0.3, chunk)[:n]
        m = ((inst == objects[k % len(objects)]) & ~drop).astype(np.uint8)
        insts.append(dict(scan_id=name, label_id=k % 18 + 1, conf=float(rng.uniform()), pred_mask=rle_encode(m)))
    gt = np.where(inst >= 0, (inst % 18 + 1) * 1000 + inst + 1, 0).astype(np.int64)
    return insts, gt


def kitti_scan(seed, n):
    _, _, inst = synthetic.scene_lidar(seed=seed, n=n)
    rng = np.random.default_rng(seed)
    cls = np.where(inst >= 0, 11 + inst % 8, rng.integers(0, 11, len(inst)))
    ids = np.where(inst >= 0, inst + 1, 0)
    return (cls | (ids << 16)).astype(np.uint32)


def median_ms(fn, reps, before=None):
    """median wall time of fn(); before() runs in front of every call, outside the timed region"""
    if before:
        before()
    fn()                                   # warm-up: code objects, pinned buffers, page cache of the directory
    times = []
    for _ in range(reps):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def event_ms(fn, reps):
    """median device time of fn's launches on the current stream"""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def device_format(insts, gt, words, reps):
    """(kernels, kernels + copy to pinned memory) in ms for one scan's text, on resident inputs"""
    lib = L.lib()
    dev = torch.device('cuda')
    jobs = []
    copies = []                            # (device text, bytes) of everything a save_* call brings to the host
    if insts:
        runs = [R._runs_of(i['pred_mask']) for i in insts]
        length = runs[0][0]
        bounds = np.zeros(len(runs) + 1, np.int64)
        np.cumsum([r[1].size for r in runs], out=bounds[1:])
        starts = torch.from_numpy(np.concatenate([r[1] for r in runs]).astype(np.int32)).to(dev)
        ends = torch.from_numpy(np.concatenate([r[2] for r in runs]).astype(np.int32)).to(dev)
        bounds_d = torch.from_numpy(bounds).to(dev)
        nbytes = len(runs) * length * 2
        text = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        jobs.append(lambda: L.check(lib.sg_mask_text_runs(
            L.ptr(starts), L.ptr(ends), L.ptr(bounds_d), int(bounds[-1]), len(runs), length, 0, len(runs), L.ptr(text),
            nbytes, L.stream()), 'sg_mask_text_runs'))
        copies.append((text, nbytes))
        n = len(gt)
        vals = torch.from_numpy(gt).to(dev)
        table = torch.tensor(NYU_ID, dtype=torch.int32, device=dev)
        gt_text = torch.empty(21 * n, dtype=torch.uint8, device=dev)
        meta = torch.empty(3, dtype=torch.int64, device=dev)
        ws = L.workspace(lib.sg_decimal_lines_workspace_bytes(n), dev)
        jobs.append(lambda: L.check(lib.sg_decimal_lines(
            L.ptr(vals), n, L.ptr(table), len(NYU_ID), L.ptr(gt_text), gt_text.numel(), L.ptr(meta), L.ptr(ws),
            ws.numel(), L.stream()), 'sg_decimal_lines'))
        jobs[-1]()
        copies.append((gt_text, int(meta.cpu()[0])))
    else:
        import ctypes as C
        table = R._kitti_table(LEARNING_MAP_INV, 19)
        lut = torch.from_numpy(table.astype(np.int32)).to(dev)
        wd = torch.from_numpy(words.view(np.int32)).to(dev)
        nbytes = 4 * len(words)
        text = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        missing = torch.empty(2, dtype=torch.int64, device=dev)
        host = (C.c_uint64 * 3)()
        jobs.append(lambda: L.check(lib.sg_panoptic_kitti_words(       # (this entry reads its count back: a sync)
            L.ptr(wd), len(words), L.ptr(lut), len(table), L.ptr(text), L.ptr(missing), C.addressof(host),
            L.stream()), 'sg_panoptic_kitti_words'))
        copies.append((text, nbytes))
    pinned = [torch.empty(max(b, 1), dtype=torch.uint8, pin_memory=True) for _, b in copies]

    def kernels():
        for j in jobs:
            j()

    def with_copy():
        kernels()
        for host, (dev_text, b) in zip(pinned, copies):
            host[:b].copy_(dev_text[:b], non_blocking=True)

    return event_ms(kernels, reps), event_ms(with_copy, reps), sum(b for _, b in copies)


def save(out, insts, gt, words, name, backend):
    if insts:
        R.save_pred_instances(out, 'pred_instance', [name], [insts], NYU_ID, backend=backend)
        R.save_gt_instances(out, 'gt_instance', [name], [gt], NYU_ID, backend=backend)
    else:
        R.save_panoptic(out, 'panoptic', [f'sequences/08/velodyne/{name}'], [words], LEARNING_MAP_INV, 19,
                        backend=backend)


def load_masks(out, name, n_masks, backend):
    got = R.load_pred_instances(os.path.join(out, 'pred_instance'), name, backend=backend)
    assert len(got) == n_masks


def load_ids(out, name, backend):
    R.read_int_lines(os.path.join(out, 'gt_instance', f'{name}.txt'), backend=backend)


def reference_method(out, insts, sample):
    """rle_decode + np.savetxt(fmt='%d') per mask (tools/test.py:52-53): median seconds per mask over `sample`
    masks, each timed on its own, after one warm-up mask"""
    os.makedirs(out, exist_ok=True)
    times = []
    for i, inst in enumerate(insts[:sample + 1]):
        t0 = time.perf_counter()
        np.savetxt(os.path.join(out, f'{i}.txt'), rle_decode(inst['pred_mask']), fmt='%d')
        times.append(time.perf_counter() - t0)
    return statistics.median(times[1:])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--ref-masks', type=int, default=5, help='masks the reference method is timed on')
    ap.add_argument('--out', default=None, help='directory to write into (default: a temporary one)')
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), 'save_results_bench.py measures the device path: it needs a GPU'
    base = args.out or tempfile.mkdtemp(prefix='save_results_bench_')
    scans = [('scannet', ) + instance_scan('scene0000_00', 1, 150000, 100) + (None, ),
             ('stpls3d', ) + instance_scan('5_points_GTv3_0', 2, 600000, 300) + (None, ),
             ('kitti', [], None, kitti_scan(3, 120000))]
    rows = []
    for kind, insts, gt, words in scans:
        out = os.path.join(base, kind)
        kernel, kernel_copy, nbytes = device_format(insts, gt, words, args.reps)
        row = dict(scan=kind, points=len(gt) if insts else len(words), masks=len(insts), text_mb=round(nbytes / 1e6, 2),
                   kernel_ms=round(kernel, 3), kernel_copy_ms=round(kernel_copy, 3))
        name = insts[0]['scan_id'] if insts else '000000'
        for backend in ('device', 'numpy'):
            ms = median_ms(lambda: save(out, insts, gt, words, name, backend), args.reps,
                           before=lambda: shutil.rmtree(out, ignore_errors=True))
            row[f'{backend}_wall_ms'] = round(ms, 2)
        if insts:                          # (the files of the last numpy run are still there)
            for backend in ('device', 'numpy'):
                ms = median_ms(lambda: load_masks(out, name, len(insts), backend), args.reps)
                row[f'read_masks_{backend}_ms'] = round(ms, 2)
                row[f'read_ids_{backend}_ms'] = round(median_ms(lambda: load_ids(out, name, backend), args.reps), 2)
        if kind == 'scannet':
            per_mask = reference_method(os.path.join(base, 'ref'), insts, args.ref_masks)
            row['reference_savetxt_ms'] = round(per_mask * len(insts) * 1e3, 1)
            row['reference_masks_timed'] = args.ref_masks
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out is None:
        shutil.rmtree(base, ignore_errors=True)
    return rows


if __name__ == '__main__':
    main()
