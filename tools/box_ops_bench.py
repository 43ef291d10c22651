"""Cost of the oriented-box operations (softgroup_amd.ops.boxes, evaluation.det_eval with get_iou_obb) on synthetic
boxes: the IoU matrix and greedy NMS of 100, 300 and 1000 boxes, and the matching of a ScanNet-val-shaped detection set
(312 images x 18 classes, about 14 GT objects and 60 detections per image).

Reported per set, all in the same run, each the median over --reps runs after a warm-up (min .. max in brackets), ms:
  event_ms        the C entry on arrays already on the device, HIP events
  device_wall_ms  host arrays in, host result out through the device (upload, kernels, read-back), wall time
  numpy_wall_ms   the vectorised numpy twin, wall time
  scalar_ms       the scalar definition in a Python loop, ONE run, over the first `scalar_pairs` pairs only (matrix),
                  the whole NMS loop / the whole reference matching loop otherwise
The device, the twin and (on its pairs) the scalar loop must agree byte for byte before anything is timed.
No polygon library is compared: none is importable here.

    python tools/box_ops_bench.py [--reps 5] [--out profiles/box_ops_bench.txt]
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
from softgroup_amd.evaluation import det_eval as de  # noqa: E402
from softgroup_amd.ops import boxes as BX  # noqa: E402

SIZES = (100, 300, 1000)
SCALAR_PAIRS = 20000
N_IMAGES, N_CLASSES, GT_PER_IMAGE, DET_PER_IMAGE = 312, 18, 14, 60
THRESHOLDS = [0.25, 0.5]


def boxes(seed, n, room=8.0):
    """n boxes of furniture size scattered over a room: a few per cent of the pairs overlap"""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(0, room, (n, 2)), rng.uniform(0.3, 1.2, (n, 1)), rng.uniform(0.3, 2.0, (n, 3)),
                           rng.uniform(-np.pi, np.pi, (n, 1))], axis=1)


def detection_set(seed):
    rng = np.random.default_rng(seed)
    pred_all, gt_all = {}, {}
    for img in range(N_IMAGES):
        g = boxes(seed * 1000 + img, GT_PER_IMAGE)
        cls = rng.integers(0, N_CLASSES, GT_PER_IMAGE)
        gt_all[img] = [(int(c), b) for c, b in zip(cls, g)]
        d = boxes(seed * 1000 + 500 + img, DET_PER_IMAGE)
        dcls = rng.integers(0, N_CLASSES, DET_PER_IMAGE)
        k = DET_PER_IMAGE // 2
        src = rng.integers(0, GT_PER_IMAGE, k)
        d[:k] = g[src] + rng.normal(0, 0.05, (k, 7))
        d[:k, 3:6] = np.abs(d[:k, 3:6])
        dcls[:k] = cls[src]
        pred_all[img] = [(int(c), b, float(s)) for c, b, s in zip(dcls, d, rng.uniform(0.05, 1, DET_PER_IMAGE))]
    return pred_all, gt_all


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


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def bench_matrix(n, reps, dev):
    a, b = BX.boxes8(boxes(1, n)), BX.boxes8(boxes(2, n))
    da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    want = BX.box_iou_numpy(a, b)
    same(BX.box_iou(da, db).cpu().numpy(), want, ('matrix', n))
    k = min(n * n, SCALAR_PAIRS)
    pairs = [(i // n, i % n) for i in range(k)]
    t0 = time.perf_counter()
    loop = np.array([BX.obb_iou_pair(a[i], b[j]) for i, j in pairs])
    scalar = [1e3 * (time.perf_counter() - t0)]
    same(loop, want.reshape(-1)[:k], ('matrix, scalar', n))

    def through_device():
        return BX.box_iou(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)).cpu().numpy()

    return dict(op='iou_matrix', boxes=n, pairs=n * n, overlapping=int((want > 0).sum()), scalar_pairs=k,
                event_ms=event_ms(lambda: BX.box_iou(da, db), reps), device_wall_ms=wall_ms(through_device, reps, True),
                numpy_wall_ms=wall_ms(lambda: BX.box_iou_numpy(a, b), reps, False), scalar_ms=scalar)


def nms_loop(rows, scores, labels, thr):
    n = len(rows)
    order = sorted(range(n), key=lambda i: (-float(scores[i]), i))
    dead, keep = set(), np.zeros(n, np.uint8)
    for pos, i in enumerate(order):
        if i in dead:
            continue
        keep[i] = 1
        for j in order[pos + 1:]:
            if j not in dead and labels[i] == labels[j] and \
                    BX.obb_iou_pair(rows[min(i, j)], rows[max(i, j)]) > thr:
                dead.add(j)
    return keep


def bench_nms(n, reps, dev):
    rng = np.random.default_rng(n)
    obb = boxes(3, n)
    obb[n // 2:] = obb[:n - n // 2] + rng.normal(0, 0.05, (n - n // 2, 7))           # every object proposed twice
    obb[:, 3:6] = np.abs(obb[:, 3:6])
    rows = BX.boxes8(obb)
    scores = rng.uniform(0.05, 1, n).astype(np.float32)
    labels = np.tile(rng.integers(0, N_CLASSES, n - n // 2), 2)[:n].astype(np.int32)
    d = [torch.from_numpy(x).to(dev) for x in (rows, scores, labels)]
    want = BX.box_nms_numpy(rows, scores, labels, 0.25)[0]
    same(BX.box_nms(*d, 0.25)[0].cpu().numpy(), want, ('nms', n))
    t0 = time.perf_counter()
    loop = nms_loop(rows, scores, labels, 0.25)
    scalar = [1e3 * (time.perf_counter() - t0)]
    same(loop, want, ('nms, scalar', n))

    def through_device():
        t = [torch.from_numpy(x).to(dev) for x in (rows, scores, labels)]
        return BX.box_nms(*t, 0.25)[0].cpu().numpy()

    return dict(op='nms', boxes=n, pairs=n * (n - 1) // 2, overlapping=int(n - want.sum()), scalar_pairs=-1,
                event_ms=event_ms(lambda: BX.box_nms(*d, 0.25), reps), device_wall_ms=wall_ms(through_device, reps, True),
                numpy_wall_ms=wall_ms(lambda: BX.box_nms_numpy(rows, scores, labels, 0.25), reps, False),
                scalar_ms=scalar)


def bench_match(reps, dev):
    pred_all, gt_all = detection_set(4)
    pred, gt = de._by_class(pred_all, gt_all)
    names = [c for c in gt if c in pred]
    jobs = [de._ClassJob(pred[c], gt[c]) for c in names]
    want = [de._match_numpy_obb(job, THRESHOLDS, '3d') for job in jobs]
    got = de._match_device(jobs, THRESHOLDS, dev, '3d')
    for w, g in zip(want, got):
        for a, b in zip(w, g):
            same(np.asarray(a, np.uint8), np.asarray(b, np.uint8), 'match')
    t0 = time.perf_counter()
    loop = [de._match_reference_loop(job, THRESHOLDS, de.get_iou_obb) for job in jobs]
    scalar = [1e3 * (time.perf_counter() - t0)]
    for w, g in zip(want, loop):
        for a, b in zip(w, g):
            same(np.asarray(a, np.uint8), np.asarray(b, np.uint8), 'match, scalar')
    # the launch pair alone, on resident arrays
    det = BX.boxes8(np.concatenate([np.asarray(j.BB, np.float64).reshape(-1, 7) for j in jobs]))
    n_det = len(det)
    sizes, group, gts = [], [], []
    for j in jobs:
        idx = {img: len(sizes) + k for k, img in enumerate(j.gt_sphere)}
        for s in j.gt_sphere.values():
            sizes.append(len(s) if s.size else 0)
            if s.size:
                gts.append(BX.boxes8(np.asarray(s, np.float64).reshape(-1, 7)))
        group += [idx[i] for i in j.image_ids]
    gtb = np.concatenate(gts)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    res = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in
           (det, np.asarray(group, np.int32), np.arange(n_det, dtype=np.int32), gtb, off)]

    def launch():
        import ctypes
        from softgroup_amd import _lib as L
        th = (ctypes.c_double * len(THRESHOLDS))(*THRESHOLDS)
        ov = torch.empty(n_det, dtype=torch.float64, device=dev)
        jm = torch.empty(n_det, dtype=torch.int64, device=dev)
        tp = torch.empty((len(THRESHOLDS), n_det), dtype=torch.uint8, device=dev)
        ws = L.workspace(L.lib().sg_det_match_obb_workspace_bytes(len(gtb), len(THRESHOLDS)), dev)
        L.check(L.lib().sg_det_match_obb(L.ptr(res[0]), L.ptr(res[1]), L.ptr(res[2]), n_det, L.ptr(res[3]), L.ptr(res[4]),
                                         len(gtb), ctypes.cast(th, ctypes.c_void_p), len(THRESHOLDS), 0, L.ptr(ov),
                                         L.ptr(jm), L.ptr(tp), L.ptr(ws), ws.numel(), L.stream()), 'sg_det_match_obb')

    launch()
    return dict(op='match', boxes=n_det, pairs=int(sum(sizes[g] for g in group)), overlapping=len(gtb), scalar_pairs=-1,
                event_ms=event_ms(launch, reps),
                device_wall_ms=wall_ms(lambda: de._match_device(jobs, THRESHOLDS, dev, '3d'), reps, True),
                numpy_wall_ms=wall_ms(lambda: [de._match_numpy_obb(j, THRESHOLDS, '3d') for j in jobs], reps, False),
                scalar_ms=scalar)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'box_ops_bench.txt'))
    args = ap.parse_args()
    dev = torch.device('cuda')
    lines = [f'# tools/box_ops_bench.py --reps {args.reps}  ({torch.cuda.get_device_name(0)}); ms, median [min .. max]; '
             f'mode 3d; scalar: one run (matrix: over the first scalar_pairs pairs only)',
             '# overlapping: pairs with IoU > 0 (matrix), suppressed boxes (nms), GT boxes (match: boxes = detections, '
             f'{N_IMAGES} images x {N_CLASSES} classes)',
             f'{"op":10s} {"boxes":>6s} {"pairs":>8s} {"overlap":>8s} {"scalar_pairs":>12s} | event | device_wall | '
             f'numpy_wall | scalar']
    rows = []
    work = [(fn, n) for fn in (bench_matrix, bench_nms) for n in SIZES] + [(bench_match, None)]
    for fn, n in work:
        r = fn(args.reps, dev) if n is None else fn(n, args.reps, dev)
        rows.append(r)
        lines.append(f'{r["op"]:10s} {r["boxes"]:6d} {r["pairs"]:8d} {r["overlapping"]:8d} {r["scalar_pairs"]:12d} | '
                     f'{cell(r["event_ms"])} | {cell(r["device_wall_ms"])} | {cell(r["numpy_wall_ms"], 1)} | '
                     f'{r["scalar_ms"][0]:.0f}')
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print(json.dumps(rows))


if __name__ == '__main__':
    main()
