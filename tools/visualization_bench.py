"""Cost of turning a test run's result tree into coloured PLY files (softgroup_amd.util.visualize) for two
synthetic scans written with save_results:

  scannet  150 000 points (synthetic.scene_s2), 100 predicted masks + the ground-truth instance ids
  stpls3d  600 000 points (synthetic.scene_s2), 300 predicted masks + the ground-truth instance ids

Per scan and task, medians over --reps runs after a warm-up run:
  format_ms       labels, colours and PLY text on resident inputs (HIP events around the launches; every input and
                  table is uploaded before the clock starts, what remains besides the kernels is the read-back of
                  the meta words after the colours and after the text, whose size is not known before)
  format_copy_ms  the same plus the copy of the text to pinned memory (events)
  device_wall_ms  save_visualizations with backend='device', call to return: inputs read, file written and closed
  numpy_wall_ms   the same with backend='numpy'
and per scan read_masks_{device,numpy}_ms: the scan's mask files into the form the paint takes (bit rows on the
device, dense arrays on the host).  Once per scan the reference's method for the vertex lines -- one format call
per vertex, restated here -- is timed on the `input` cloud: reference_format_ms (text built and written).

    python tools/visualization_bench.py [--reps 5] [--out DIR]
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
from softgroup_amd import synthetic  # noqa: E402
from softgroup_amd.util import results as R  # noqa: E402
from softgroup_amd.util import visualize as V  # noqa: E402
from softgroup_amd.util.rle import rle_encode  # noqa: E402


class Dataset:
    NYU_ID = (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39)


def scan_result(name, seed, n, n_masks, chunk=200):
    """a forward_test result dict: predicted masks = an object's points with chunks of consecutive points removed"""
    xyz, rgb, inst = synthetic.scene_s2(seed=seed, n=n)
    n = len(inst)
    rng = np.random.default_rng(seed)
    objects = np.unique(inst[inst >= 0])
    insts = []
    for k in range(n_masks):
        drop = np.repeat(rng.uniform(size=n // chunk + 1) < 0.3, chunk)[:n]
        m = ((inst == objects[k % len(objects)]) & ~drop).astype(np.uint8)
        insts.append(dict(scan_id=name, label_id=k % 18 + 1, conf=float(rng.uniform()), pred_mask=rle_encode(m)))
    sem = np.where(inst >= 0, inst % 18 + 2, rng.integers(0, 2, n))
    sem[rng.uniform(size=n) < 0.05] = -100
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    offsets = f32(rng.standard_normal((n, 3)) * 0.1)
    return dict(scan_id=name, coords_float=f32(xyz), color_feats=f32(rgb), semantic_labels=sem.astype(np.int64),
                semantic_preds=np.where(sem < 0, 0, sem).astype(np.int64), offset_preds=offsets, offset_labels=offsets,
                gt_instances=np.where(inst >= 0, (inst % 18 + 1) * 1000 + inst + 1, 0).astype(np.int64),
                pred_instances=insts)


def median_ms(fn, reps, before=None):
    if before:
        before()
    fn()                                   # warm-up: code objects, pinned buffers, page cache
    times = []
    for _ in range(reps):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def event_ms(fn, reps):
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


class _Resident(V._Stage):
    """a stage whose uploads are made once: the kernels are timed on resident inputs.  The scan's arrays are
    known by identity, the small tables that are rebuilt per call (priority, skip) by content."""

    def __init__(self):
        super().__init__()
        self.kept = {}

    def upload(self, a, dtype):
        a = np.asarray(a)
        key = (a.tobytes() if a.nbytes <= 65536 else id(a), a.dtype.str, np.dtype(dtype).str)
        if key not in self.kept:
            self.kept[key] = (a, super().upload(a, dtype))
        return self.kept[key][1]


def device_format(scan, task, reps):
    """(format_ms, format_copy_ms, bytes of text) for one cloud"""
    stage = _Resident()
    n = len(scan['coords'])
    inst, cls = V.INSTANCE_PALETTE, V.SCANNET_CLASS_PALETTE
    keep_host = np.ascontiguousarray(scan['semantic_label'] != -100, dtype=np.uint8)
    scan.cache['keep8'] = keep_host
    if task == 'instance_pred':
        scan['instances']                                  # (the mask files are read before the clock starts)

    def kernels(copy=False):
        rgb, _ = V._rgb_device(stage, scan, task, inst, cls)
        xyz = stage.upload(scan['coords'], np.float32)
        offset = stage.upload(scan['offset_pred'], np.float32) if task == 'offset_semantic_pred' else None
        keep = stage.upload(scan.cache['keep8'], np.uint8)
        pinned, _, total, _, declined = V._vertex_text_device(stage, xyz, offset, rgb, keep, n)
        assert declined == 0
        if copy:
            pinned[:total].copy_(stage.text[:total], non_blocking=True)
        return total

    total = kernels()
    return event_ms(kernels, reps), event_ms(lambda: kernels(True), reps), total


def reference_method(path, xyz, colors):
    """the reference's way to the vertex lines: a Python loop over the vertices with one format call each
    (numpy scalars in, as there), text written to `path`: seconds"""
    t0 = time.perf_counter()
    scaled = colors * 255
    with open(path, 'w') as f:
        f.write(V._HEADER % (len(xyz), 0))
        for i in range(len(xyz)):
            x, y, z = xyz[i]
            r, g, b = scaled[i]
            f.write('%f %f %f %d %d %d\n' % (x, y, z, int(r), int(g), int(b)))
    return time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None, help='directory to write into (default: a temporary one)')
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), 'visualization_bench.py measures the device path: it needs a GPU'
    base = args.out or tempfile.mkdtemp(prefix='visualization_bench_')
    rows = []
    for kind, name, seed, n, n_masks in (('scannet', 'scene0000_00', 1, 150000, 100),
                                         ('stpls3d', '5_points_GTv3_0', 2, 600000, 300)):
        result = scan_result(name, seed, n, n_masks)
        root, ply = os.path.join(base, kind, 'results'), os.path.join(base, kind, 'ply')
        R.save_results(root, [result], ['semantic', 'instance'], Dataset)
        points = len(result['gt_instances'])
        for backend in ('device', 'numpy'):
            stage = V._Stage() if backend == 'device' else None
            ms = median_ms(lambda: V._file_instances(root, name, points, backend, stage), args.reps)
            row = dict(scan=kind, points=points, masks=n_masks, what=f'read_masks_{backend}_ms', ms=round(ms, 2))
            rows.append(row)
            print(json.dumps(row), flush=True)
        resident = V._file_scan(root, name, 'device', V._Stage())
        for task in V.TASKS:
            kernel, kernel_copy, nbytes = device_format(resident, task, args.reps)
            row = dict(scan=kind, points=points, masks=n_masks, task=task, text_mb=round(nbytes / 1e6, 2),
                       format_ms=round(kernel, 3), format_copy_ms=round(kernel_copy, 3))
            for backend in ('device', 'numpy'):
                ms = median_ms(lambda: V.save_visualizations(root, [name], [task], ply, backend=backend), args.reps,
                               before=lambda: shutil.rmtree(ply, ignore_errors=True))
                row[f'{backend}_wall_ms'] = round(ms, 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
        xyz, rgb = V.get_coords_color(root, name, 'input', backend='numpy')
        times = [reference_method(os.path.join(base, kind, 'ref.ply'), xyz, rgb / 255) for _ in range(3)]
        row = dict(scan=kind, points=points, vertices=len(xyz), what='reference_format_ms',
                   ms=round(statistics.median(times[1:]) * 1e3, 1), runs_timed=2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out is None:
        shutil.rmtree(base, ignore_errors=True)
    return rows


if __name__ == '__main__':
    main()
