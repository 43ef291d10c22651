"""Cost of snapping masks and labels to superpoints (softgroup_amd.util.snap_instances / refine_result,
ops.superpoint) on synthetic instance lists: synthetic.scene_s2 clouds of 150 k points with 100 masks and of 600 k
points with 300 masks.  Superpoints are voxel cells of 0.1 m (the ``inverse`` of voxel_downsample); a mask is 90 % of
the points of one object plus 30 stray points anywhere; RLE dicts, what forward_test returns; labels are the object
ids with 15 % noise.  thr 0.5, 'snap'.

Reported per cloud, all in the same run, each the median over --reps runs after a warm-up:
  index_ms         sg_superpoint_index on ids already on the device, from HIP events (the read-back of meta included)
  snap_ms          sg_mask_snap on bit rows already on the device, from HIP events
  vote_ms          sg_superpoint_vote on labels already on the device, from HIP events
  *_numpy_ms       the numpy twin of the same operation, wall time
  snap_instances   util.snap_instances(backend='device' | 'numpy'), wall time: RLE text in, RLE text out
  refine_result    util.refine_result(backend='device' | 'numpy'), wall time: index + vote + snap_instances
The two backends must return the same results, byte for byte, before anything is timed.

    python tools/superpoint_bench.py [--reps 5] [--out profiles/superpoint_bench.txt]
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
from softgroup_amd.data import voxel_downsample  # noqa: E402
from softgroup_amd.ops import superpoint as SP  # noqa: E402
from softgroup_amd.util import masks as UM  # noqa: E402
from softgroup_amd.util import refine_result, snap_instances  # noqa: E402
from softgroup_amd.util.rle import rle_encode  # noqa: E402

CASES = [('scannet', 150000, 1.0, 100), ('stpls3d', 600000, 2.0, 300)]
VOXEL, THR, MODE, N_CLASSES = 0.1, 0.5, 'snap', 20


def make_case(seed, n_points, room_scale, n_masks):
    xyz, _, inst = synthetic.scene_s2(seed=seed, n=n_points, room_scale=room_scale)
    rng = np.random.default_rng(seed)
    n_obj = int(inst.max()) + 1
    insts = []
    for k in range(n_masks):
        m = (inst == k % n_obj) & (rng.random(xyz.shape[0]) < 0.9)
        m[rng.integers(xyz.shape[0], size=30)] = True
        insts.append(dict(scan_id='s', label_id=int(1 + k % 18), conf=float(f'{rng.uniform():.4f}'),
                          pred_mask=rle_encode(m.astype(np.int64))))
    sem = np.where(inst >= 0, inst % N_CLASSES, -100).astype(np.int64)
    noise = rng.random(sem.size) < 0.15
    sem[noise] = rng.integers(0, N_CLASSES, size=int(noise.sum()))
    sp = np.asarray(voxel_downsample(xyz, VOXEL, backend='numpy')[1]).astype(np.int32)
    return sp, insts, sem


def wall_ms(fn, reps, sync=True):
    ts = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def event_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def same_lists(a, b):
    return len(a) == len(b) and all(x == y for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'superpoint_bench.txt'))
    args = ap.parse_args()
    dev = torch.device('cuda')
    head = ('set', 'points', 'masks', 'segs', 'index', 'index_numpy', 'snap', 'snap_numpy', 'vote', 'vote_numpy',
            'snap_inst_dev', 'snap_inst_numpy', 'refine_dev', 'refine_numpy')
    lines = [f'# tools/superpoint_bench.py --reps {args.reps}  ({torch.cuda.get_device_name(0)}); ms, median; '
             f"voxel {VOXEL}, thr {THR}, '{MODE}', {N_CLASSES} classes",
             ' '.join(f'{h:>{max(len(h), 8)}s}' for h in head)]
    rows = []
    for c, (name, n_points, room_scale, n_masks) in enumerate(CASES):
        sp, insts, sem = make_case(30 + c, n_points, room_scale, n_masks)
        result = dict(scan_id='s', semantic_preds=sem, pred_instances=insts)
        d_sp, d_sem = torch.from_numpy(sp).to(dev), torch.from_numpy(sem).to(dev)
        # ---- equality first (also the warm-up)
        h_idx, d_idx = SP.superpoint_index(sp), SP.superpoint_index(d_sp)
        assert (h_idx.n_seg, h_idx.n_valid, h_idx.max_size) == (d_idx.n_seg, d_idx.n_valid, d_idx.max_size)
        for a, b in zip((h_idx.order, h_idx.seg_of, h_idx.seg_start), (d_idx.order, d_idx.seg_of, d_idx.seg_start)):
            assert np.array_equal(a, b.cpu().numpy()), name
        packed = UM.packed_rows(insts, n_points)
        bits = torch.from_numpy(packed.view(np.int32)).to(dev)
        h_snap = SP.mask_snap_numpy(packed, n_points, h_idx, THR, MODE)
        d_snap = SP.mask_snap(bits, n_points, d_idx, THR, MODE)
        assert np.array_equal(h_snap[0], d_snap[0].cpu().numpy()) and np.array_equal(h_snap[1], d_snap[1].cpu().numpy())
        assert not np.array_equal(h_snap[0], packed.view(np.int32)), 'the masks must have something to snap'
        h_vote = SP.superpoint_vote_numpy(sem, h_idx, N_CLASSES)
        assert np.array_equal(h_vote, SP.superpoint_vote(d_sem, d_idx, N_CLASSES).cpu().numpy())
        want = refine_result(result, sp, n_classes=N_CLASSES, backend='numpy')
        got = refine_result(result, d_sp, n_classes=N_CLASSES, backend='device')
        assert np.array_equal(want['semantic_preds'], got['semantic_preds'])
        assert same_lists(want['pred_instances'], got['pred_instances']), name
        assert same_lists(snap_instances(insts, d_idx, THR, MODE, backend='device'), want['pred_instances'])
        # ---- times
        row = dict(set=name, points=n_points, masks=n_masks, segs=h_idx.n_seg)
        row['index'] = event_ms(lambda: SP.superpoint_index(d_sp), args.reps)
        row['index_numpy'] = wall_ms(lambda: SP.superpoint_index_numpy(sp), args.reps, sync=False)
        row['snap'] = event_ms(lambda: SP.mask_snap(bits, n_points, d_idx, THR, MODE), args.reps)
        row['snap_numpy'] = wall_ms(lambda: SP.mask_snap_numpy(packed, n_points, h_idx, THR, MODE), args.reps,
                                    sync=False)
        row['vote'] = event_ms(lambda: SP.superpoint_vote(d_sem, d_idx, N_CLASSES), args.reps)
        row['vote_numpy'] = wall_ms(lambda: SP.superpoint_vote_numpy(sem, h_idx, N_CLASSES), args.reps, sync=False)
        row['snap_inst_dev'] = wall_ms(lambda: snap_instances(insts, d_idx, THR, MODE, backend='device'), args.reps)
        row['snap_inst_numpy'] = wall_ms(lambda: snap_instances(insts, h_idx, THR, MODE, backend='numpy'), args.reps,
                                         sync=False)
        kw = dict(n_classes=N_CLASSES)
        row['refine_dev'] = wall_ms(lambda: refine_result(result, d_sp, backend='device', **kw), args.reps)
        row['refine_numpy'] = wall_ms(lambda: refine_result(result, sp, backend='numpy', **kw), args.reps, sync=False)
        rows.append(row)
        cells = [f'{row[h]:>{max(len(h), 8)}.3f}' if isinstance(row[h], float) else f'{row[h]!s:>{max(len(h), 8)}s}'
                 for h in head]
        lines.append(' '.join(cells))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print(json.dumps(rows))


if __name__ == '__main__':
    main()
