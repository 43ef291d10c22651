"""Cost of combining K results over one cloud (softgroup_amd.util.ensemble_results) on scene_s2 clouds: 150 k points
with about 100 masks per pass and 600 k points with about 300, K = 4 and K = 8 passes.

A pass reports the points of the cells of a coarse grid as its instances (RLE dicts; the points of a cell are
scattered over the index range, so a mask has about as many runs as points), perturbed per pass: every mask eroded by
a point stride that depends on the pass, one instance dropped, one duplicated; its labels are the cell's class with
10 % of the points flipped.

Timed, each the median of --reps runs after a warm-up, all in one run:
  label vote        device_kernel_ms  sg_label_vote on a resident [K, N] tensor, from HIP events (no read-back)
                    device_wall_ms    the vote of ensemble_results(backend='device') on numpy labels (upload, kernel,
                                      download), wall time
                    numpy_wall_ms     the same with backend='numpy'
  instances         device_kernel_ms  sg_mask_group_links + sg_stitch_components + the read-back of the components +
                                      sg_mask_vote + the read-back of the populations on resident bit rows, from events
                    device_wall_ms / numpy_wall_ms of the whole call (RLE dicts in, RLE dicts out)
                    naive_wall_ms     what a user writes today: decode every RLE to a dense mask, loop over the
                                      pairs and the objects in Python -- one run; null where the pair loop alone is
                                      estimated (from its first 200 pairs) to take more than a minute
The device and numpy results are compared for equality before anything is timed.

    python tools/ensemble_bench.py [--reps 5] [--out profiles/ensemble_bench.txt]
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
from softgroup_amd.ops import ensemble as EN  # noqa: E402
from softgroup_amd.ops import stitch as ST  # noqa: E402
from softgroup_amd.util import ensemble as UE  # noqa: E402
from softgroup_amd.util import ensemble_results, masks as M, rle_decode  # noqa: E402
from softgroup_amd.util.rle import rle_encode_runs  # noqa: E402

CLOUDS = [(150000, 1.0, 0.55), (600000, 2.0, 0.63)]      # points, room scale, side of the coarse cells (m)
PASSES = (4, 8)


def median_ms(fn, reps, events=False, warm=True):
    if warm:
        fn()
    wall, dev = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(e0.elapsed_time(e1))
    return (float(np.median(wall)), float(np.median(dev))) if events else float(np.median(wall))


def make_passes(xyz, side, k, seed=0):
    """k result dicts over the cloud"""
    rng = np.random.default_rng(seed)
    n = xyz.shape[0]
    cell = np.floor(xyz[:, :2].astype(np.float64) / side).astype(np.int64)
    blob = (cell[:, 1] - cell[:, 1].min()) * (cell[:, 0].max() - cell[:, 0].min() + 1) + (cell[:, 0] - cell[:, 0].min())
    order = np.argsort(blob, kind='stable')
    groups = np.split(order, np.flatnonzero(np.diff(blob[order])) + 1)
    idx = np.arange(n)
    results = []
    for p in range(k):
        insts = []
        for j, grp in enumerate(groups):
            if j == p:
                continue                                            # dropped by this pass
            b = int(blob[grp[0]])
            for copy in range(2 if j == p + 1 else 1):              # duplicated by this pass
                keep = np.sort(grp[(idx[grp] + p + copy) % (7 + p) != 0]) if p else np.sort(grp)
                if keep.size == 0:
                    continue
                head = np.concatenate([[True], np.diff(keep) > 1])
                starts = keep[head]
                ends = keep[np.concatenate([head[1:], [True]])] + 1
                insts.append(dict(scan_id='bench', label_id=1 + b % 18, conf=0.2 + 1e-4 * b + 1e-6 * p,
                                  pred_mask=rle_encode_runs(n, starts, ends - starts)))
        sem = (blob % 18 + 1).astype(np.int64)
        flip = rng.random(n) < 0.1
        sem[flip] = rng.integers(0, 19, int(flip.sum()))
        results.append(dict(scan_id='bench', semantic_preds=sem, pred_instances=insts))
    return results


def naive(results, thr=0.5):
    """dense masks and Python loops; -> (instances, None) or (None, estimated seconds of the pair loop)"""
    k = len(results)
    flat = [(p, inst) for p, r in enumerate(results) for inst in r['pred_instances']]
    dense = [rle_decode(inst['pred_mask']).astype(bool) for _, inst in flat]
    pairs = [(g, h) for g in range(len(flat)) for h in range(g + 1, len(flat))
             if flat[g][0] != flat[h][0] and flat[g][1]['label_id'] == flat[h][1]['label_id']]
    parent = list(range(len(flat)))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    t0 = time.perf_counter()
    for done, (g, h) in enumerate(pairs):
        if done == 200:
            estimate = (time.perf_counter() - t0) / 200 * len(pairs)
            if estimate > 60.0:
                return None, estimate
        inter = int((dense[g] & dense[h]).sum())
        union = int(dense[g].sum()) + int(dense[h].sum()) - inter
        if union and inter >= 1 and inter / union > thr:
            a, b = find(g), find(h)
            parent[max(a, b)] = min(a, b)
    members = {}
    for g in range(len(flat)):
        members.setdefault(find(g), []).append(g)
    out = []
    for root in sorted(members):
        m = members[root]
        passes = sorted({flat[g][0] for g in m})
        if len(passes) < k // 2 + 1:
            continue
        votes = np.zeros(dense[0].size, np.int32)
        for p in passes:
            held = np.zeros(dense[0].size, bool)
            for g in m:
                if flat[g][0] == p:
                    held |= dense[g]
            votes += held
        out.append((flat[m[0]][1]['label_id'], votes >= len(passes) // 2 + 1))
    return out, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ensemble_bench.txt'))
    args = ap.parse_args()
    dev = torch.device('cuda', torch.cuda.current_device())
    lines = [f'device {torch.cuda.get_device_name(0)}; scene_s2 clouds, K passes with unit weights, thr 0.5 iou, '
             f"mask 'majority'; ms, medians of {args.reps} after a warm-up (naive: one run)"]
    print(lines[0], flush=True)
    for n, room_scale, side in CLOUDS:
        xyz, _, _ = synthetic.scene_s2(seed=1, n=n, room_scale=room_scale)
        for k in PASSES:
            results = make_passes(np.ascontiguousarray(xyz, np.float32), side, k)
            n_inst = sum(len(r['pred_instances']) for r in results)
            a = ensemble_results(results, backend='device')
            b = ensemble_results(results, backend='numpy')
            assert [(i['label_id'], i['conf'], i['pred_mask']) for i in a['pred_instances']] == \
                [(i['label_id'], i['conf'], i['pred_mask']) for i in b['pred_instances']]
            assert np.array_equal(a['semantic_preds'], b['semantic_preds'])

            # ---- label vote
            labels_only = [dict(semantic_preds=r['semantic_preds']) for r in results]
            d_labels = torch.from_numpy(np.stack([r['semantic_preds'] for r in results])).to(dev)
            _, lab_kernel = median_ms(lambda: EN.label_vote(d_labels), args.reps, events=True)
            lab_dev = median_ms(lambda: ensemble_results(labels_only, backend='device'), args.reps)
            lab_np = median_ms(lambda: ensemble_results(labels_only, backend='numpy'), args.reps)
            row = dict(op='label_vote', points=n, passes=k, device_kernel_ms=round(lab_kernel, 3),
                       device_wall_ms=round(lab_dev, 3), numpy_wall_ms=round(lab_np, 3))
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)

            # ---- instances
            inst_only = [dict(pred_instances=r['pred_instances']) for r in results]
            per_pass = [r['pred_instances'] for r in results]
            bits = torch.cat([M.checked_rows_device(pi, n, dev) for pi in per_pass])
            insts = [i for pi in per_pass for i in pi]
            group = np.repeat(np.arange(k), [len(pi) for pi in per_pass]).astype(np.int32)
            labels = np.array([i['label_id'] for i in insts], np.int32)
            weights = np.ones(k, np.int64)

            def kernels():
                adj = EN.mask_group_links(bits, n, labels, group)
                comp = ST.stitch_components(adj, len(insts)).cpu().numpy()
                objects, need = UE._kept_objects(comp, group, weights, k // 2 + 1, 'majority')
                EN.mask_vote(bits, n, *EN.member_lists(objects, group, weights), need)[1].cpu()

            _, inst_kernel = median_ms(kernels, args.reps, events=True)
            inst_dev, inst_event = median_ms(lambda: ensemble_results(inst_only, backend='device'), args.reps, events=True)
            inst_np = median_ms(lambda: ensemble_results(inst_only, backend='numpy'), args.reps, warm=False)
            t0 = time.perf_counter()
            got, estimate = naive(results)
            naive_ms = (time.perf_counter() - t0) * 1e3 if got is not None else None
            if got is not None:
                assert [g[0] for g in got] == [i['label_id'] for i in b['pred_instances']]
                assert all(int(g[1].sum()) == int(rle_decode(i['pred_mask']).sum())
                           for g, i in zip(got, b['pred_instances']))
            row = dict(op='instances', points=n, passes=k, instances=n_inst, objects=len(b['pred_instances']),
                       device_kernel_ms=round(inst_kernel, 3), device_event_ms=round(inst_event, 3),
                       device_wall_ms=round(inst_dev, 3), numpy_wall_ms=round(inst_np, 3),
                       naive_wall_ms=None if naive_ms is None else round(naive_ms, 3),
                       naive_pair_loop_estimate_s=None if estimate is None else round(estimate, 1))
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
            del bits, d_labels

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
