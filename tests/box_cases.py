"""The shared generators of the oriented-box tests (a helper, not collected): exact rotations, the degenerate list,
random box lists, detection sets and a synthetic scan.  test_box_ops.py holds the numpy twins of
``softgroup_amd.ops.boxes`` to the scalar definition, to exact arithmetic and to plain loops on these cases;
test_box_ops_gpu.py holds the device to the twins."""
from fractions import Fraction

import numpy as np

from softgroup_amd.ops import boxes as BX

TRIPLES = ((3, 4, 5), (5, 12, 13), (8, 15, 17), (7, 24, 25), (20, 21, 29))
HALF = Fraction(1, 2)


def rotations():
    """(c, s) as exact fractions: the five triples with every sign and both swaps, and the four axis cases"""
    out = [(Fraction(1), Fraction(0)), (Fraction(0), Fraction(1)), (Fraction(-1), Fraction(0)),
           (Fraction(0), Fraction(-1))]
    for a, b, h in TRIPLES:
        for x, y in ((a, b), (b, a)):
            for sx in (1, -1):
                for sy in (1, -1):
                    out.append((Fraction(sx * x, h), Fraction(sy * y, h)))
    return out


def exact_pairs(seed, n):
    """n pairs of rectangles as exact rows (cx, cy, cz, du, dv, dz, c, s) of Fractions: centres and extents are
    multiples of 1/64, rotations come from ``rotations``"""
    rng = np.random.default_rng(seed)
    rots = rotations()

    def row():
        cx, cy = (Fraction(int(v), 64) for v in rng.integers(-96, 97, 2))
        du, dv = (Fraction(int(v), 64) for v in rng.integers(1, 193, 2))
        c, s = rots[int(rng.integers(len(rots)))]
        return [cx, cy, Fraction(0), du, dv, Fraction(1), c, s]

    return [(row(), row()) for _ in range(n)]


def to_float(row):
    return np.array([float(v) for v in row], dtype=np.float64)


def exact_area(a, b):
    """the rules of ``area(a, b)`` in exact arithmetic (written apart from the code under test)"""
    poly = []
    for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
        u, v = su * HALF * a[3], sv * HALF * a[4]
        x, y = a[0] + (u * a[6] - v * a[7]), a[1] + (u * a[7] + v * a[6])
        dx, dy = x - b[0], y - b[1]
        poly.append((dx * b[6] + dy * b[7], dy * b[6] - dx * b[7]))
    for axis, sign, h in ((0, 1, HALF * b[3]), (0, -1, HALF * b[3]), (1, 1, HALF * b[4]), (1, -1, HALF * b[4])):
        out = []
        for i, p in enumerate(poly):
            q = poly[(i + 1) % len(poly)]
            dp, dq = h - sign * p[axis], h - sign * q[axis]
            if dp >= 0:
                out.append(p)
            if (dp >= 0) != (dq >= 0):
                t = dp / (dp - dq)
                r = [p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])]
                r[axis] = sign * h
                out.append(tuple(r))
        poly = out
        if not poly:
            return Fraction(0)
    if len(poly) < 3:
        return Fraction(0)
    x0, y0 = poly[0]
    acc = Fraction(0)
    for i in range(1, len(poly) - 1):
        acc += (poly[i][0] - x0) * (poly[i + 1][1] - y0) - (poly[i + 1][0] - x0) * (poly[i][1] - y0)
    return abs(acc) * HALF


def random_obb(seed, n, spread=2.0):
    """n random boxes (cx, cy, cz, du, dv, dz, theta), close enough to overlap often"""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-spread, spread, (n, 2)), rng.uniform(-0.5, 0.5, (n, 1)),
                           rng.uniform(0.2, 2.0, (n, 3)), rng.uniform(-4.0, 4.0, (n, 1))], axis=1)


# (a, b, what the 3D IoU must be: a number, or None for "positive, below 1")
R2 = np.sqrt(2.0)
DEGENERATE = [
    ('identical', [0.5, -0.25, 1, 2, 1, 3, 0.3], [0.5, -0.25, 1, 2, 1, 3, 0.3], None),
    ('shared_edge', [0, 0, 0, 2, 2, 2, 0], [2, 0, 0, 2, 2, 2, 0], 0.0),
    ('shared_corner', [0, 0, 0, 2, 2, 2, 0], [2, 2, 0, 2, 2, 2, 0], 0.0),
    ('containment', [0, 0, 0, 4, 4, 4, 0], [0.25, 0.5, 0, 1, 2, 2, 0.7], 1 * 2 * 2 / (4 * 4 * 4)),
    ('contained', [0.25, 0.5, 0, 1, 2, 2, 0.7], [0, 0, 0, 4, 4, 4, 0], 1 * 2 * 2 / (4 * 4 * 4)),
    ('zero_du', [0, 0, 0, 0, 2, 2, 0.2], [0, 0, 0, 2, 2, 2, 0], 0.0),
    ('zero_dv', [0, 0, 0, 2, 0, 2, 0.2], [0, 0, 0, 2, 2, 2, 0], 0.0),
    ('zero_dz', [0, 0, 0, 2, 2, 0, 0.2], [0, 0, 0, 2, 2, 2, 0], 0.0),
    ('both_zero', [0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0], 0.0),
    ('z_touch', [0, 0, 0, 2, 2, 2, 0.4], [0, 0, 2, 2, 2, 2, 0.4], 0.0),
    ('z_apart', [0, 0, 0, 2, 2, 2, 0.4], [0, 0, 5, 2, 2, 2, 0.4], 0.0),
    ('far_apart', [0, 0, 0, 2, 2, 2, 0.4], [1e6, -1e6, 0, 2, 2, 2, 1.1], 0.0),
    ('octagon', [0, 0, 0, 1, 1, 1, 0], [0, 0, 0, 1, 1, 1, np.pi / 4], None),
    ('cross', [0, 0, 0, 4, 1, 1, 0], [0, 0, 0, 1, 4, 1, 0], 1.0 / 7.0),
]


def degenerate_rows():
    """-> (a [k, 8], b [k, 8]) box rows of the degenerate list"""
    a = BX.boxes8(np.array([d[1] for d in DEGENERATE], dtype=np.float64))
    b = BX.boxes8(np.array([d[2] for d in DEGENERATE], dtype=np.float64))
    return a, b


def mixed_rows(seed, n):
    """n box rows: random boxes with the boxes of the degenerate list mixed in at random places (as many as fit)"""
    rows = BX.boxes8(random_obb(seed, n))
    if n:
        rng = np.random.default_rng(seed + 1000)
        a, b = degenerate_rows()
        special = np.concatenate([a, b])[rng.permutation(2 * len(DEGENERATE))][:n]
        rows[rng.choice(n, size=len(special), replace=False)] = special
    return rows


def invalid_rows():
    """box rows that must raise: a NaN, an infinity and a negative extent, each in an otherwise good row"""
    good = BX.boxes8(random_obb(5, 4))
    out = []
    for col, val in ((0, np.nan), (2, np.inf), (3, -1.0), (4, -1e-300), (5, -np.inf), (6, np.nan), (7, np.inf)):
        r = good.copy()
        r[1, col] = val
        out.append(r)
    return good, out


def nms_loop(rows, scores, labels, thr, mode, class_agnostic):
    """greedy NMS as a plain double loop over the scalar definition -> keep uint8 [n]"""
    n = len(rows)
    scores = np.asarray(scores, np.float32)
    order = sorted(range(n), key=lambda i: (-float(scores[i]), i))
    dead, keep = set(), np.zeros(n, np.uint8)
    for pos, i in enumerate(order):
        if i in dead:
            continue
        keep[i] = 1
        for j in order[pos + 1:]:
            if j in dead or not (class_agnostic or labels is None or labels[i] == labels[j]):
                continue
            lo, hi = min(i, j), max(i, j)
            if BX.obb_iou_pair(rows[lo], rows[hi], mode) > thr:
                dead.add(j)
    return keep


def detection_set(seed, n_img=3, n_gt=5, n_det=12):
    """(pred, gt) of one class for eval_det_cls with 7-number boxes: images without GT, an image whose GT list holds
    the same box twice, detections that copy a GT box, detections of equal confidence, a group of one"""
    rng = np.random.default_rng(seed)
    pred, gt = {}, {}
    for img in range(n_img):
        g = random_obb(seed * 100 + img, n_gt if img else 1)
        if img == 1:
            g[2] = g[0]                                        # duplicate GT: the first wins
        gt[img] = [row for row in g]
        d = random_obb(seed * 100 + 50 + img, n_det)
        k = min(len(g), n_det)
        d[:k] = g[:k] + rng.normal(0, 0.03, (k, 7))            # near copies of the GT boxes
        d[k:k + 2] = g[0]                                      # two exact copies: one GT for both
        conf = np.round(rng.uniform(0.05, 1.0, n_det), 1)      # one decimal: equal confidences occur
        pred[img] = [(d[i], float(conf[i])) for i in range(n_det)]
    pred[n_img] = [(random_obb(seed + 7, 1)[0], 0.5)]          # detections in an image without GT
    gt[n_img + 1] = [random_obb(seed + 8, 1)[0]]               # GT in an image without detections
    return pred, gt


def match_inputs(seed, n_det, n_groups, max_gt, mode='3d'):
    """arrays for sg_det_match_obb / match_boxes: box rows, groups (some empty, one of a single GT, one with a
    duplicated GT), ranks with the detections of a group copying its GT boxes"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, max_gt + 1, n_groups)
    if n_groups > 2:
        sizes[0], sizes[1], sizes[2] = 0, 1, max(2, sizes[2])
    gt = random_obb(seed + 1, int(sizes.sum()))
    off = np.concatenate([[0], np.cumsum(sizes)])
    if n_groups > 2:
        gt[off[2] + 1] = gt[off[2]]                            # duplicate GT
    det = random_obb(seed + 2, n_det)
    group = rng.integers(0, max(n_groups, 1), n_det).astype(np.int32)
    for d in range(n_det):
        g = group[d]
        if sizes[g] and d % 3:
            det[d] = gt[off[g] + rng.integers(sizes[g])]
            if d % 3 == 2:
                det[d, :6] += rng.normal(0, 0.02, 6) * (np.arange(6) < 3)
    rank = rng.permutation(n_det).astype(np.int32)
    return BX.boxes8(det), group, rank, BX.boxes8(gt), sizes.astype(np.int64)


def match_loop(det, group, rank, gt, sizes, ths, mode):
    """the reference loop on those arrays -> (ovmax, jmax, tp [n_thr, n_det])"""
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = len(det)
    ov, jm = np.full(n, -np.inf), np.full(n, -1, np.int64)
    for d in range(n):
        for j in range(off[group[d]], off[group[d] + 1]):
            iou = BX.obb_iou_pair(det[d], gt[j], mode)
            if iou > ov[d]:
                ov[d], jm[d] = iou, j
    tp = np.zeros((len(ths), n), np.uint8)
    for k, t in enumerate(ths):
        taken = set()
        for d in np.argsort(rank, kind='stable'):
            if ov[d] > t and jm[d] not in taken:
                tp[k, d] = 1
                taken.add(jm[d])
    return ov, jm, tp


def synthetic_scan(seed=3, n_points=20000, n_masks=40):
    """a scan for evaluate_box_ap and nms_boxes: coords float32, semantic and instance labels, predictions with
    dense masks (objects of the scene with a tenth of their points dropped, every fifth mask two objects)"""
    from softgroup_amd import synthetic
    xyz, rgb, inst = synthetic.scene_s2(seed=seed, n=n_points)
    n = xyz.shape[0]
    rng = np.random.default_rng(seed)
    n_obj = int(inst.max()) + 1
    sem = np.where(inst >= 0, 2 + np.maximum(inst, 0) % 18, 0).astype(np.int64)
    preds = []
    for k in range(n_masks):
        objs = rng.choice(n_obj, size=2 if k % 5 == 4 else 1, replace=False)
        m = np.isin(inst, objs) & (rng.random(n) < 0.9)
        preds.append(dict(scan_id='s', label_id=int(1 + objs[0] % 18), conf=float(f'{rng.uniform():.4f}'),
                          pred_mask=m))
    return dict(coords=np.ascontiguousarray(xyz, dtype=np.float32), colors=np.ascontiguousarray(rgb, np.float32),
                semantic=sem, instance=inst.astype(np.int64), preds=preds,
                class_labels=[f'class{i}' for i in range(18)])
