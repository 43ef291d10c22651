"""Cost of ScanNetEval (softgroup_amd.evaluation) after a test run, host backend against device backend
in the same run, on two synthetic result sets:

  scannet  32 scans of 150 000 points, about 100 predicted masks (RLE dicts) and 30 GT instances each
  stpls3d   8 scans of 600 000 points, about 300 predicted masks and 100 GT instances each

Medians over --reps evaluations after one warm-up evaluation:
  host_ms_per_scan      evaluate(backend='host'), wall time / scans (its count matrix runs on the GPU)
  device_ms_per_scan    evaluate(backend='device'), wall time / scans, compute() included
  update_enqueue_ms     wall time of one update() call (it returns once the scan's work is enqueued)
  update_device_ms      device time of one scan's copies and kernels (HIP events around the update loop)
  compute_ms            wall time of compute(): the sorts and curves of all scans and the read-back
For a few scans of the first set the reference's association -- a dense 0/1 mask per prediction and
np.logical_and per same-class (prediction, GT) pair -- is timed as well.  The averages of both backends
are compared before anything is reported.

    python tools/inst_eval_bench.py [--reps 5] [--write]      (--write: profiles/inst_eval_bench.txt)

--coverage measures what ScanNetEval(coverage=True) (mCov / mWCov / mPrec / mRec) adds instead: on the same two
sets the device path's three figures with the metrics off, on, and off again (the second "off" shows the noise
of the run), the host path's wall time off and on, and the four averages of both paths, which must be equal to
the bit.  It writes profiles/coverage_eval_bench.txt.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from softgroup_amd.evaluation import ScanNetEval  # noqa: E402
from softgroup_amd.util.rle import rle_decode, rle_encode  # noqa: E402

CLASSES = tuple(f'class{i}' for i in range(18))


def make_scan(name, seed, n_points, n_inst, n_false):
    """GT instances = contiguous blocks with holes; per instance 0-5 predictions keeping part of it plus stray
    points, mostly with its class; n_false predictions elsewhere"""
    rng = np.random.default_rng(seed)
    gts = np.zeros(n_points, np.int64)
    cuts = np.sort(rng.choice(np.arange(1000, n_points - 1000), n_inst * 2, replace=False))
    preds = []
    for i in range(n_inst):
        lo, hi = cuts[2 * i], cuts[2 * i + 1]
        m = np.zeros(n_points, bool)
        m[lo:hi] = np.repeat(rng.random((hi - lo) // 50 + 1) < 0.9, 50)[:hi - lo]
        cls = int(rng.integers(1, 19))
        gts[m] = cls * 1000 + i + 1
        idx = np.flatnonzero(m)
        for _ in range(int(rng.integers(0, 6))):
            pm = np.zeros(n_points, bool)
            pm[idx[np.repeat(rng.random(len(idx) // 20 + 1) < rng.uniform(0.3, 1.0), 20)[:len(idx)]]] = True
            pm[rng.integers(0, n_points, int(rng.uniform(0, 0.05) * len(idx)))] = True
            label = cls if rng.random() < 0.85 else int(rng.integers(1, 19))
            preds.append(dict(scan_id=name, label_id=label, conf=float(rng.random()), pred_mask=rle_encode(pm.astype(np.uint8))))
    for _ in range(n_false):
        pm = np.zeros(n_points, bool)
        a = int(rng.integers(0, n_points - 5000))
        pm[a:a + int(rng.integers(150, 5000))] = True
        preds.append(dict(scan_id=name, label_id=int(rng.integers(1, 19)), conf=float(rng.random()),
                          pred_mask=rle_encode(pm.astype(np.uint8))))
    return preds, gts


def median_wall_ms(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def device_parts(ev, pl, gl, reps):
    """(update enqueue wall, update device time, compute wall) in ms; the first two per scan"""
    enq, dev, comp = [], [], []
    for r in range(reps + 1):
        ev.reset(backend='device')
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        for preds, gts in zip(pl, gl):
            ev.update(preds, gts)
        t1 = time.perf_counter()
        b.record()
        b.synchronize()
        t2 = time.perf_counter()
        ev.compute()
        t3 = time.perf_counter()
        assert ev.last_backend == 'device', ev.last_fallback
        if r:                                      # the first round is the warm-up
            enq.append((t1 - t0) * 1e3 / len(pl))
            dev.append(a.elapsed_time(b) / len(pl))
            comp.append((t3 - t2) * 1e3)
    return statistics.median(enq), statistics.median(dev), statistics.median(comp)


def reference_association_ms(preds, gts):
    """the reference's method for one scan: dense masks, logical_and per same-class pair"""
    t0 = time.perf_counter()
    ids = np.unique(gts)
    ids = ids[(ids // 1000 >= 1) & (ids // 1000 <= 18)]
    gt_masks = {int(i): gts == i for i in ids}
    for p in preds:
        m = rle_decode(p['pred_mask']).astype(bool)
        for i, g in gt_masks.items():
            if i // 1000 == p['label_id']:
                np.count_nonzero(np.logical_and(g, m))
    return (time.perf_counter() - t0) * 1e3


def same(a, b):
    if isinstance(b, dict):
        return set(a) == set(b) and all(same(a[k], b[k]) for k in b)
    a, b = float(a), float(b)
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-12


def coverage_main(args, sets):
    rows = []
    for kind, n_scans, n_points, n_inst, n_false in sets:
        made = [make_scan(f'{kind}{s}', 100 + s, n_points, n_inst, n_false) for s in range(n_scans)]
        pl, gl = [m[0] for m in made], [m[1] for m in made]
        off, on = ScanNetEval(list(CLASSES)), ScanNetEval(list(CLASSES), coverage=True)
        host = on.evaluate(pl, gl, verbose=False, backend='host')
        dev = on.evaluate(pl, gl, verbose=False, backend='device')
        assert on.last_backend == 'device', on.last_fallback
        keys = ('all_cov', 'all_wcov', 'all_prec', 'all_rec')
        assert all(float(host[k]).hex() == float(dev[k]).hex() for k in keys), 'device and host coverage differ'
        assert all(np.array_equal(v, dev['coverage_counts'][k]) for k, v in host['coverage_counts'].items())
        assert same({k: v for k, v in dev.items() if k != 'coverage_counts'},
                    {k: v for k, v in host.items() if k != 'coverage_counts'}), 'device and host averages differ'
        row = dict(set=kind, scans=n_scans, points=n_points,
                   preds_per_scan=round(sum(len(p) for p in pl) / n_scans, 1), gt_per_scan=n_inst)
        row.update({'host_' + k: float(host[k]) for k in keys})
        row.update({'device_' + k: float(dev[k]) for k in keys})
        for tag, ev in (('off', off), ('on', on), ('off_again', off)):
            enq, dms, comp = device_parts(ev, pl, gl, args.reps)
            row.update({f'update_enqueue_ms_{tag}': round(enq, 3), f'update_device_ms_{tag}': round(dms, 3),
                        f'compute_ms_{tag}': round(comp, 3)})
        for tag, ev in (('off', off), ('on', on)):
            row[f'host_ms_per_scan_{tag}'] = round(median_wall_ms(
                lambda: ev.evaluate(pl, gl, verbose=False, backend='host'), args.reps) / n_scans, 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
    path = os.path.join(ROOT, 'profiles', 'coverage_eval_bench.txt')
    with open(path, 'w') as f:
        arch = getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?').split(':')[0]
        f.write(f'tools/inst_eval_bench.py --coverage --reps {args.reps} on {torch.cuda.get_device_name(0)} ({arch})\n')
        f.write('medians after one warm-up; ScanNetEval with coverage=None (off, off_again) and coverage=True (on) '
                'timed in the same run; update figures per scan\n')
        for row in rows:
            f.write(json.dumps(row) + '\n')
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--ref-scans', type=int, default=2, help='scans the reference association is timed on')
    ap.add_argument('--write', action='store_true', help='write profiles/inst_eval_bench.txt')
    ap.add_argument('--coverage', action='store_true',
                    help='cost of coverage=True against coverage=None; writes profiles/coverage_eval_bench.txt')
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), 'inst_eval_bench.py measures the device path: it needs a GPU'
    sets = [('scannet', 32, 150000, 30, 25), ('stpls3d', 8, 600000, 100, 50)]
    if args.coverage:
        return coverage_main(args, sets)
    rows = []
    for kind, n_scans, n_points, n_inst, n_false in sets:
        made = [make_scan(f'{kind}{s}', 100 + s, n_points, n_inst, n_false) for s in range(n_scans)]
        pl, gl = [m[0] for m in made], [m[1] for m in made]
        ev = ScanNetEval(list(CLASSES))
        host = ev.evaluate(pl, gl, verbose=False, backend='host')
        dev = ev.evaluate(pl, gl, verbose=False, backend='device')
        assert ev.last_backend == 'device', ev.last_fallback
        assert same(dev, host), 'device and host averages differ'
        row = dict(set=kind, scans=n_scans, points=n_points,
                   preds_per_scan=round(sum(len(p) for p in pl) / n_scans, 1), gt_per_scan=n_inst,
                   all_ap=round(float(host['all_ap']), 4))
        row['host_ms_per_scan'] = round(median_wall_ms(
            lambda: ev.evaluate(pl, gl, verbose=False, backend='host'), args.reps) / n_scans, 3)
        row['device_ms_per_scan'] = round(median_wall_ms(
            lambda: ev.evaluate(pl, gl, verbose=False, backend='device'), args.reps) / n_scans, 3)
        enq, dms, comp = device_parts(ev, pl, gl, args.reps)
        row.update(update_enqueue_ms=round(enq, 3), update_device_ms=round(dms, 3), compute_ms=round(comp, 3))
        if kind == 'scannet':
            ref = [reference_association_ms(p, g) for p, g in list(zip(pl, gl))[:args.ref_scans + 1]]
            row['reference_association_ms_per_scan'] = round(statistics.median(ref[1:]), 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.write:
        path = os.path.join(ROOT, 'profiles', 'inst_eval_bench.txt')
        with open(path, 'w') as f:
            arch = getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?').split(':')[0]
            f.write(f'tools/inst_eval_bench.py --reps {args.reps} on {torch.cuda.get_device_name(0)} ({arch})\n')
            f.write('medians after one warm-up; host and device backends timed in the same run\n')
            for row in rows:
                f.write(json.dumps(row) + '\n')
    return rows


if __name__ == '__main__':
    main()
