"""Cost of box detection AP (evaluate_box_ap) on a synthetic ScanNet-like set: 16 scans x 150 k points,
40 GT instances and 100 predicted masks (RLE, as forward_test returns them) per scan, %.4f confidences,
thresholds 0.25 and 0.5.

Reported per scan, each the median over --reps runs:
  device: the whole device path, split into the host-to-device copy of coordinates and labels, box
    extraction (RLE parsing on the host, sg_det_boxes_runs + sg_det_boxes_labels), matching
    (sg_det_match for both thresholds) and the host AP (regrouping, argsort, cumsum, voc_ap);
  numpy: the numpy path (device='cpu');
  reference_loop: the reference script's own way, in one process -- coords[mask] per decoded mask,
    instance_label == i per GT instance, get_iou per (detection, GT) pair in the Python double loop,
    once per threshold -- and that figure times 312 (ScanNet val).

    python tools/box_eval_bench.py [--reps 5] [--scans 16]
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
from softgroup_amd.evaluation import det_eval as de  # noqa: E402
from softgroup_amd.evaluation import evaluate_box_ap  # noqa: E402
from softgroup_amd.util.rle import rle_decode, rle_encode  # noqa: E402

CLASSES = ['cabinet', 'bed', 'chair', 'sofa', 'table', 'door', 'window', 'bookshelf', 'picture', 'counter', 'desk',
           'curtain', 'refrigerator', 'shower curtain', 'toilet', 'sink', 'bathtub', 'otherfurniture']
THS = (0.25, 0.5)


def scan(seed, n=150000, n_gt=40, n_pred=100, chunk=500):
    """instances as boxes of points, laid out in chunks of `chunk` consecutive points (mesh vertex
    order keeps an object's points in few runs) plus background; predictions = a GT instance's points
    with some removed, as the RLE dicts forward_test returns"""
    rng = np.random.default_rng(seed)
    n_chunks = n // chunk
    owner = np.where(rng.uniform(size=n_chunks) < 0.5, rng.integers(0, n_gt, n_chunks), -100)
    owner[:n_gt] = np.arange(n_gt)
    inst = np.repeat(owner, chunk).astype(np.int64)
    lo = rng.uniform(0, 8, (n_gt, 3))
    hi = lo + rng.uniform(0.3, 2.0, (n_gt, 3))
    xyz = rng.uniform(0, 10, (n, 3))
    o = inst >= 0
    t = rng.uniform(size=(int(o.sum()), 3))
    xyz[o] = lo[inst[o]] + t * (hi - lo)[inst[o]]
    cls = rng.integers(2, 20, n_gt)
    sem = np.where(o, cls[np.maximum(inst, 0)], rng.integers(0, 2, n)).astype(np.int64)
    preds = []
    for p in range(n_pred):
        g = rng.integers(0, n_gt)
        m = (inst == g) & np.repeat(rng.uniform(size=n_chunks) < 0.9, chunk)
        m[np.flatnonzero(inst == g)[0]] = True
        label = int(cls[g if rng.uniform() < 0.8 else rng.integers(0, n_gt)]) - 1    # some mislabelled
        preds.append(dict(scan_id=f'scene{seed:04d}_00', label_id=label, conf=float(f'{rng.uniform():.4f}'),
                          pred_mask=rle_encode(m.astype(np.int64))))
    return xyz.astype(np.float32), sem, inst, preds


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


def reference_loop(preds, coords, sems, insts):
    """the reference script's work in one process: boxes per decoded mask and per instance id, then
    eval_sphere's Python double loop (get_iou per pair) once per threshold"""
    pred_all, gt_all = {}, {}
    for s, (ps, c, sem, inst) in enumerate(zip(preds, coords, sems, insts)):
        pr = []
        for p in ps:
            pts = c[rle_decode(p['pred_mask']).astype(bool)]
            pr.append((CLASSES[p['label_id'] - 1], np.concatenate([pts.min(0), pts.max(0)]), p['conf']))
        gt = []
        for i in range(int(inst.max()) + 1):
            sel = inst == i
            cls_id = int(sem[np.nonzero(sel)[0][0]])
            if cls_id >= 2:
                pts = c[sel]
                gt.append((CLASSES[cls_id - 2], np.concatenate([pts.min(0), pts.max(0)])))
        pred_all[s], gt_all[s] = pr, gt
    for t in THS:
        de._eval_multi(pred_all, gt_all, [t], False, lambda a, b: de.get_iou(a, b), 'cpu', 'zero')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--scans', type=int, default=16)
    args = ap.parse_args()
    warnings.simplefilter('ignore', RuntimeWarning)
    data = [scan(100 + s) for s in range(args.scans)]
    coords, sems, insts, preds = [list(x) for x in zip(*data)]
    S = args.scans
    masks = [[p['pred_mask'] for p in ps] for ps in preds]

    def full(device):
        return evaluate_box_ap(preds, coords, sems, insts, CLASSES, iou_thresholds=THS, device=device)

    a, b = full('cuda'), full('cpu')                                  # warm-up, and the two paths agree
    assert all(a[t]['mAP'] == b[t]['mAP'] for t in THS), (a, b)
    dev = timed(lambda: full('cuda'), args.reps)
    h2d = timed(lambda: [torch.from_numpy(x).to('cuda') for x in coords + insts], args.reps)
    boxes = timed(lambda: de.instance_boxes(coords, masks, insts, device='cuda'), args.reps)

    # matching and host AP on the boxes the device formed
    pb, gts = de.instance_boxes(coords, masks, insts, device='cuda')
    pred_all = {s: [(CLASSES[p['label_id'] - 1], pb[s][k], p['conf']) for k, p in enumerate(preds[s])]
                for s in range(S)}
    gt_all = {}
    for s, (gb, cnt, first) in enumerate(gts):
        gt_all[s] = [(CLASSES[int(sems[s][first[i]]) - 2], gb[i]) for i in range(len(cnt))
                     if sems[s][first[i]] >= 2]
    pred, gt = de._by_class(pred_all, gt_all)
    names = [c for c in gt if c in pred]

    def jobs():
        return [de._ClassJob(pred[c], gt[c]) for c in names]
    js = jobs()
    match = timed(lambda: de._match_device(js, THS, 'cuda'), args.reps)
    flags = de._match_device(js, THS, 'cuda')
    host_ap = timed(lambda: [[j.finish(f, False) for f in fl] for j, fl in zip(jobs(), flags)], args.reps, sync=False)
    numpy_s = timed(lambda: full('cpu'), max(1, args.reps // 2), sync=False)
    ref_s = timed(lambda: reference_loop(preds, coords, sems, insts), 1, sync=False)

    n_det = sum(len(p) for p in preds)
    out = dict(scans=S, points_per_scan=150000, detections=n_det, gt=sum(len(g) for g in gt_all.values()),
               device_ms_per_scan=1e3 * dev / S, device_h2d_ms_per_scan=1e3 * h2d / S,
               device_boxes_ms_per_scan=1e3 * (boxes - h2d) / S, device_match_ms_per_scan=1e3 * match / S,
               host_ap_ms_per_scan=1e3 * host_ap / S, numpy_ms_per_scan=1e3 * numpy_s / S,
               reference_loop_ms_per_scan=1e3 * ref_s / S, reference_loop_312_scans_s=ref_s / S * 312,
               mAP_25=float(a[0.25]['mAP']), mAP_50=float(a[0.5]['mAP']))
    print(' '.join(f'{k}={v:.3f}' if isinstance(v, float) else f'{k}={v}' for k, v in out.items()))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
