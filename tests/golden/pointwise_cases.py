"""Deterministic inputs for the point-wise evaluators (semantic mIoU / accuracy, offset MAE) and
PanopticEval, shared by tests/golden/make_pointwise_golden.py (which runs the REFERENCE's evaluators
on them) and the tests.  They cover: ignored points, predicted classes absent from the ground truth,
a gt class with no correct point, an all-ignored scan, offsets with ignored instances, thing-only
and stuff-only class lists, a pred segment spanning two gt instances, a pair at IoU exactly 0.5,
segments just below and at min_points, panoptic ids up to 0xFFFF, the fusion's ignore value
(class = n_classes), instance labels below -1, scans of different sizes and an empty prediction
set.  ``kitti_like`` / ``scannet_like`` also make the large synthetic sets of the GPU tests and of
tools/eval_bench.py."""
import numpy as np

IGNORE = -100


# ------------------------------------------------------------------ semantic / offsets
def scannet_like(seed, n, n_classes=20, ignore_frac=0.1, noise=0.2):
    """(sem_pred int64, sem_gt int64, offset_pred f32 [n,3], offset_gt f32 [n,3], inst int64)"""
    rng = np.random.default_rng(seed)
    gt = rng.integers(0, n_classes, n)
    gt[rng.random(n) < ignore_frac] = IGNORE
    pred = np.where(rng.random(n) < noise, rng.integers(0, n_classes, n), np.maximum(gt, 0))
    inst = rng.integers(0, 40, n)
    inst[rng.random(n) < 0.3] = IGNORE
    og = (rng.standard_normal((n, 3)) * 0.5).astype(np.float32)
    op = (og + rng.standard_normal((n, 3)) * 0.1).astype(np.float32)
    return pred.astype(np.int64), gt.astype(np.int64), op, og, inst.astype(np.int64)


def semantic_cases():
    """name -> (pred_list, gt_list, offset_pred_list, offset_gt_list, inst_list)"""
    a = scannet_like(1, 5000)
    b = scannet_like(2, 1234)
    pred, gt = a[0].copy(), a[1].copy()
    pred[pred == 7] = 8                      # class 7: in the gt, never a correct point
    gt[gt == 11] = 12                        # class 11: predicted, absent from the gt
    a = (pred, gt) + a[2:]
    c = scannet_like(3, 300)
    c = (c[0], np.full(300, IGNORE, np.int64), c[2], c[3], np.full(300, IGNORE, np.int64))   # all ignored
    out = {}
    for name, scans in (('three_scans', [a, b, c]), ('one_scan', [b]), ('all_ignored', [c])):
        out[name] = tuple(list(x) for x in zip(*scans))
    return out


# ------------------------------------------------------------------ panoptic
N_CLASSES = 6                                # stuff 0..2, thing 3..5; fusion ignore value = 6
STUFF = ['road', 'sidewalk', 'vegetation']
THING = ['car', 'person', 'cyclist']


def _pan(cls, ids):
    return (np.asarray(ids, np.uint32) << 16) | np.asarray(cls, np.uint32)


def designed_scan():
    """one scan whose segments hit the edge cases one by one -> (pred uint32, sem int64, inst int64)"""
    sem, inst, pcls, pid = [], [], [], []

    def block(n, s, i, c, k):
        sem.append(np.full(n, s)); inst.append(np.full(n, i)); pcls.append(np.full(n, c)); pid.append(np.full(n, k))

    block(180, 0, IGNORE, 0, 0)              # stuff 0: one segment (ignored instances -> y = 1)
    block(20, 0, IGNORE, 1, 0)               #   ... partly predicted as stuff 1
    block(150, 1, IGNORE, 1, 0)
    block(100, 2, IGNORE, 2, 0)
    block(30, 2, IGNORE, 4, 7)               # class 4 predicted where no gt of class 4 exists
    block(70, 3, 10, 3, 1)                   # pred id 1 spans gt 10 (70) and gt 11 (50): TP with 10 only
    block(50, 3, 11, 3, 1)
    block(30, 5, 20, 5, 2)                   # pred 2 = 30 of gt 20 (40) + all of gt 21 (20): IoU 30/60 = 0.5
    block(20, 5, 21, 5, 2)
    block(10, 5, 20, 5, 3)
    block(49, 5, 22, N_CLASSES, 0)           # gt 22: 49 points, unmatched, below min_points: no FN
    block(50, 5, 23, N_CLASSES, 0)           # gt 23: 50 points, unmatched: an FN
    block(49, 2, IGNORE, 3, 4)               # pred 4: 49 points of class 3 on stuff: no FP
    block(50, 2, IGNORE, 3, 5)               # pred 5: 50 points: an FP
    block(80, 3, 24, 3, 0xFFFF)              # the largest id
    block(25, 3, -5, 3, 0xFFFF)              # instance labels below -1: y <= 0, no gt segment
    block(15, 3, -1, 3, 9)                   # instance -1: y = 1, like the ignored ones
    block(30, IGNORE, 3, 3, 1)               # void points: never counted
    block(12, 4, IGNORE, 0, 0)               # (gt class 4 with no correct point)
    cat = np.concatenate
    return _pan(cat(pcls), cat(pid)), cat(sem).astype(np.int64), cat(inst).astype(np.int64)


def kitti_like(seed, n, n_classes=19, n_stuff=11, n_inst=60, ignore_frac=0.05):
    """a LiDAR-like scan: stuff background, n_inst thing instances as runs of points, predictions that
    mostly agree with shifted boundaries, merges, splits, class noise and the fusion's ignore value
    -> (pred uint32, sem int64, inst int64)"""
    rng = np.random.default_rng(seed)
    sem = rng.integers(0, n_stuff, n).astype(np.int64)
    sem = np.repeat(sem[: n // 64 + 1], 64)[:n]              # stuff in runs
    inst = np.full(n, IGNORE, np.int64)
    pcls = sem.copy()
    pid = np.zeros(n, np.int64)
    max_size = min(1500, n // 4)
    starts = np.sort(rng.choice(n - max_size, n_inst, replace=False))
    next_id = 1
    for k, s in enumerate(starts):
        size = int(rng.integers(20, max_size))
        c = int(rng.integers(n_stuff, n_classes))
        sem[s:s + size] = c
        inst[s:s + size] = k
        lo = s + int(rng.integers(-size // 4, size // 4 + 1))
        hi = s + size + int(rng.integers(-size // 4, size // 4 + 1))
        lo, hi = max(lo, 0), min(max(hi, lo + 1), n)
        pcls[lo:hi] = c
        mode = rng.random()
        if mode < 0.1:                                        # no id: the fusion's ignore value
            pcls[lo:hi] = n_classes
        elif mode < 0.2:                                      # split in two
            mid = (lo + hi) // 2
            pid[lo:mid], pid[mid:hi] = next_id, next_id + 1
            next_id += 2
        else:
            pid[lo:hi] = next_id
            next_id += 1 if mode < 0.9 else 0                 # ... or merged into the next one
    noise = rng.random(n) < 0.05
    pcls[noise] = rng.integers(0, n_classes, int(noise.sum()))
    pid[noise & (pcls < n_stuff)] = 0
    sem[rng.random(n) < ignore_frac] = IGNORE
    inst[rng.random(n) < 0.01] = -1
    return _pan(pcls, pid), sem, inst


def panoptic_cases():
    """name -> (thing, stuff, kwargs, [pred], [sem], [inst])"""
    d = designed_scan()
    k1 = kitti_like(11, 3000, n_classes=N_CLASSES, n_stuff=3, n_inst=12)
    k2 = kitti_like(12, 1777, n_classes=N_CLASSES, n_stuff=3, n_inst=8)
    empty = (np.full(900, N_CLASSES, np.uint32), k2[1][:900].copy(), k2[2][:900].copy())   # no pred segment
    none = (np.zeros(0, np.uint32), np.zeros(0, np.int64), np.zeros(0, np.int64))          # a scan of no points
    scans = [d, k1, k2, empty, none]
    lists = [list(x) for x in zip(*scans)]
    return {
        'kitti': (THING, STUFF, {}, *lists),
        'min_points_30': (THING, STUFF, dict(min_points=30), *lists),
        'thing_only': (STUFF + THING, [], {}, *lists),
        'stuff_only': ([], STUFF + THING, {}, *lists),
        'designed': (THING, STUFF, {}, [d[0]], [d[1]], [d[2]]),
        'empty_preds': (THING, STUFF, {}, [empty[0]], [empty[1]], [empty[2]]),
    }
