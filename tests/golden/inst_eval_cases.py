"""Deterministic inputs for the device path of ScanNetEval, shared by
tests/golden/make_inst_eval_golden.py (which runs the REFERENCE's ScanNetEval on them) and
tests/test_inst_eval*.py: five small scans (3 000 - 5 000 points, at most 16 GT instances and 40
predictions each) that between them take every branch of the matcher:

scan 0 (hand-built)
  * one prediction covering two same-class GTs with IoU 0.5 each: at threshold 0.25 the first GT visits
    it, the second skips it and becomes a hard false negative; at 0.5 and above it is a false positive
  * four predictions on one GT (duplicates), one of them with the highest score coming last
  * a TP and an FP with the same confidence; a -0.0 / 0.0 pair on one GT
  * a GT of 60 points (below the default minimum of 100, above 30) with a prediction of IoU 0.6 on it
  * a GT of a class that is not evaluated (25); a prediction wholly on it (ignored)
  * predictions with ignore proportion 0.49 and exactly 0.5 (false positives from 0.5 on only)
  * a prediction with an invalid label (40, kept in class-agnostic mode) and one of 50 points (too small)
  * class 11: GT but never a prediction (AP 0); classes 4 and 6: predictions but never a GT (NaN);
    class 18: neither
scan 1: GT instances, no predictions.   scan 2: predictions, no GT instance (unannotated + class 25).
scans 3, 4: random blocks with partial, shifted and mislabelled predictions."""
import numpy as np

from eval_cases import CLASSES, _rle  # noqa: F401

CONFIGS = {'class_aware': dict(use_label=True), 'class_agnostic': dict(use_label=False),
           'min_npoint_30': dict(use_label=True, min_npoint=30)}
GT_CLASSES = (1, 2, 3, 5, 7, 8, 9, 10, 12, 13)          # never 4, 6 (predictions only), 11 (hand-built only), 18
PRED_LABELS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13)  # never 11, 18


def _pred(scan, n, ranges, label, conf, as_rle):
    m = np.zeros(n, bool)
    for lo, hi in ranges:
        m[lo:hi] = True
    return dict(scan_id=scan, label_id=int(label), conf=np.float32(conf),
                pred_mask=_rle(m) if as_rle else m.astype(np.int32))


def _hand_built(as_rle):
    n = 4000
    gts = np.zeros(n, np.int64)
    for cls, inst, lo, hi in ((3, 1, 0, 200), (3, 2, 200, 400), (5, 3, 500, 1000), (7, 4, 1100, 1400),
                              (2, 5, 1500, 2000), (9, 6, 2100, 2160), (25, 7, 2200, 2500), (11, 8, 2500, 3000),
                              (3, 9, 3100, 3400)):
        gts[lo:hi] = cls * 1000 + inst
    P = lambda *a: _pred('hand', n, *a, as_rle)  # noqa: E731
    preds = [
        P([(0, 400)], 3, 0.8),                       # two GTs, IoU 0.5 each
        P([(500, 1000)], 5, 0.9), P([(500, 950)], 5, 0.7), P([(500, 800)], 5, 0.6), P([(520, 1000)], 5, 0.95),
        P([(1100, 1400)], 7, 0.5), P([(1500, 1700)], 7, 0.5),      # TP and FP, same confidence
        P([(1500, 2000)], 2, -0.0), P([(1500, 1800)], 2, 0.0),
        P([(2060, 2160)], 9, 0.65),                  # 60 of its 100 points on the small GT, 40 unannotated
        P([(2200, 2500)], 4, 0.4),                   # wholly on the class that is not evaluated
        P([(2451, 2551)], 4, 0.3),                   # ignore proportion 0.49
        P([(2450, 2550)], 6, 0.3),                   # ignore proportion 0.5
        P([(3100, 3300), (3350, 3400)], 3, 0.75),    # two runs
        P([(3600, 3900)], 40, 0.8),                  # label not evaluated
        P([(3100, 3150)], 3, 0.99),                  # too small
        P([], 3, 0.97),                              # empty mask
    ]
    return preds, gts


def _random(seed, n, n_inst, as_rle):
    rng = np.random.default_rng(seed)
    gts = np.zeros(n, np.int64)
    edges = np.sort(rng.choice(np.arange(1, n // 50), n_inst * 2, replace=False)) * 50
    inst = []
    for i in range(n_inst):
        lo, hi = int(edges[2 * i]), int(edges[2 * i + 1])
        m = np.zeros(n, bool)
        m[lo:hi] = rng.random(hi - lo) < 0.9
        cls = int(rng.choice(GT_CLASSES)) if i != 4 else 25
        gts[m] = cls * 1000 + i + 1
        inst.append((m, cls))
    preds = []
    for m, cls in inst:
        idx = np.flatnonzero(m)
        for _ in range(int(rng.integers(0, 3))):
            pm = np.zeros(n, bool)
            pm[idx[rng.random(len(idx)) < rng.uniform(0.3, 1.0)]] = True
            pm[rng.integers(0, n, int(rng.uniform(0, 0.5) * len(idx)))] = True
            label = cls if (rng.random() < 0.8 and cls in PRED_LABELS) else int(rng.choice(PRED_LABELS))
            preds.append(dict(scan_id=f'rand{seed}', label_id=label,
                              conf=np.float32(rng.choice([0.3, 0.5, 0.5, 0.7, rng.random()])),
                              pred_mask=_rle(pm) if as_rle else pm.astype(np.int32)))
    for _ in range(4):
        a = int(rng.integers(0, n - 600))
        preds.append(_pred(f'rand{seed}', n, [(a, a + int(rng.integers(110, 600)))], rng.choice(PRED_LABELS),
                           rng.random(), as_rle))
    order = rng.permutation(len(preds))
    return [preds[i] for i in order], gts


def cases(as_rle=True):
    pl, gl = [], []
    p, g = _hand_built(as_rle)
    pl.append(p), gl.append(g)
    g = np.zeros(3000, np.int64)                    # GT instances, no predictions
    g[100:400], g[400:700], g[1000:1050] = 3001, 5002, 7003
    pl.append([]), gl.append(g)
    g = np.zeros(3500, np.int64)                    # predictions, no GT instance
    g[2000:2500] = 25001
    pl.append([_pred('nogt', 3500, [(0, 300)], 3, 0.6, as_rle), _pred('nogt', 3500, [(1900, 2100)], 5, 0.7, as_rle)])
    gl.append(g)
    for seed, n in ((7, 5000), (8, 4500)):
        p, g = _random(seed, n, 14, as_rle)
        pl.append(p), gl.append(g)
    return pl, gl
