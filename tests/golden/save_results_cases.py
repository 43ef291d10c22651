"""Deterministic inputs of the result-file golden (save_results_golden.json, written by
make_save_results_golden.py from the reference's tools/test.py save_* functions).  numpy only.

cases(): name -> dict with
    kind     'pred' | 'gt' | 'panoptic' | 'npy'
    args     the arguments of the matching save_* function after (root, name) -- for 'npy' a dict
             {directory name: arrays} saved with one save_npy call each
    tiny     True: the golden stores the files' bytes, not only size and SHA-256
    raises   'KeyError' when the reference raises it (the unmapped panoptic class)
masks(name): for the 'pred' cases, the dense masks the run-length dicts were encoded from, per scan.
"""
import numpy as np

NYU_ID = (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39)
# learning_map_inv of SemanticKITTI's semantic-kitti.yaml
LEARNING_MAP_INV = {0: 0, 1: 10, 2: 11, 3: 15, 4: 18, 5: 20, 6: 30, 7: 31, 8: 32, 9: 40, 10: 44, 11: 48, 12: 49,
                    13: 50, 14: 51, 15: 70, 16: 71, 17: 72, 18: 80, 19: 81}
KITTI_CLASSES = 19
INT64_MAX, INT64_MIN = 2**63 - 1, -2**63


def rle(mask):
    """the reference's wire format: 1-based 'start len start len ...'"""
    m = np.concatenate([[0], np.asarray(mask, dtype=np.uint8), [0]])
    edges = np.flatnonzero(m[1:] != m[:-1]) + 1
    edges[1::2] -= edges[::2]
    return dict(length=int(len(mask)), counts=' '.join(str(int(x)) for x in edges))


def _random_mask(rng, n, segments, longest):
    m = np.zeros(n, dtype=np.uint8)
    for _ in range(segments):
        lo = int(rng.integers(0, n))
        m[lo:lo + int(rng.integers(1, longest + 1))] = 1
    return m


def _special_masks(n):
    """empty, full, first point, last point, runs that end on 32-point word boundaries, runs that start there"""
    z = lambda: np.zeros(n, dtype=np.uint8)  # noqa: E731
    empty, full, first, last, word_end, word_start, checker = z(), z() + 1, z(), z(), z(), z(), z()
    first[0] = 1
    last[n - 1] = 1
    for w in (1, 2, 5, 40, n // 32):
        word_end[max(32 * w - 7, 0):32 * w] = 1          # ..., 32 w - 1 | 32 w free
    word_end[0:32] = 1
    for w in (3, 4, 9, 77):
        if 32 * w < n:
            word_start[32 * w:32 * w + 33] = 1           # a whole word and the next word's first point
    checker[::2] = 1
    return [empty, full, first, last, word_end, word_start, checker]


_CONFS = [0.12345, 0.12344999, 0.99995, 0.99994999, 0.00005, 0.00004999, 1.0, 0.5, 0.0, 0.33335, 0.66665,
          np.float32(0.12345), np.float32(0.99995), np.float32(0.7), 0.99999, 0.1]


def _scan(scan_id, masks, seed):
    rng = np.random.default_rng(seed)
    insts = []
    for i, m in enumerate(masks):
        conf = _CONFS[i % len(_CONFS)] if i < 2 * len(_CONFS) else float(rng.random())
        insts.append(dict(scan_id=scan_id, label_id=i % 18 + 1, conf=conf, pred_mask=rle(m)))
    return insts


def _scannet_masks():
    rng = np.random.default_rng(11)
    a = []                                                                   # 2000 points: 8 | n, 32 !| n
    b_mask = np.zeros(4992, dtype=np.uint8)                                  # 4992 = 32 * 156
    for w in (1, 7, 8, 100, 156):
        b_mask[32 * w - 5:32 * w] = 1
    n = 4099                                                                 # 8 !| n
    c = _special_masks(n)
    while len(c) < 40:
        c.append(_random_mask(rng, n, int(rng.integers(1, 30)), int(rng.integers(1, 400))))
    return {'scene0000_00': (2000, a), 'scene0011_01': (4992, [b_mask]), 'scene0704_00': (n, c)}


def _many_masks():
    rng = np.random.default_rng(12)
    n = 2003
    out = []
    for _ in range(1005):
        m = np.zeros(n, dtype=np.uint8)
        m[rng.integers(0, n, size=int(rng.integers(1, 6)))] = 1
        out.append(m)
    return {'5_points_GTv3_0': (n, out)}


def _tiny_masks():
    return {'tiny': (13, [np.array([1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1], np.uint8), np.zeros(13, np.uint8),
                          np.ones(13, np.uint8)]),
            'one': (1, [np.ones(1, np.uint8), np.zeros(1, np.uint8)])}


_PRED = {'pred_scannet': (_scannet_masks, NYU_ID, False), 'pred_plain': (_scannet_masks, None, False),
         'pred_1005': (_many_masks, None, False), 'pred_tiny': (_tiny_masks, NYU_ID, True)}


def masks(name):
    return {k: v[1] for k, v in _PRED[name][0]().items()}


def _gt_ids(seed, n):
    rng = np.random.default_rng(seed)
    sem = rng.integers(0, 19, size=n)
    ins = rng.integers(0, 1000, size=n)
    sem[:40] = np.repeat([1, 18, 0, 9], 10)
    ins[:40:10] = 999
    ins[1:40:10] = 0
    v = sem * 1000 + ins
    v[rng.random(n) < 0.2] = 0                   # ignore points (get_gt_instances writes 0)
    return v.astype(np.int64)


def _powers():
    v = [0, 1, -1]
    for k in range(1, 19):
        v += [10**k - 1, 10**k, -(10**k - 1), -(10**k)]
    v += [10**18 * 9, INT64_MAX, INT64_MIN, INT64_MAX - 1, INT64_MIN + 1, 2**32, 2**32 - 1, -2**32, 2**31, -2**31]
    return np.array(v, dtype=np.int64)


def _kitti_words(seed, n):
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, KITTI_CLASSES + 1, size=n).astype(np.uint32)
    cls[:20] = np.arange(20)
    ids = rng.integers(0, 0x10000, size=n).astype(np.uint32)
    ids[:4] = [0, 0xFFFF, 1, 0x8000]
    return (cls | (ids << np.uint32(16))).astype(np.uint32)


def _semantic_arrays(seed, n):
    rng = np.random.default_rng(seed)
    f3 = lambda: rng.standard_normal((n, 3)).astype(np.float32)  # noqa: E731
    return dict(coords=f3(), colors=f3(), semantic_pred=rng.integers(0, 20, size=n).astype(np.int64),
                semantic_label=rng.integers(-100, 20, size=n).astype(np.int64), offset_pred=f3(), offset_label=f3())


def cases():
    c = {}
    for name, (build, nyu, tiny) in _PRED.items():
        scans = build()
        ids = list(scans)
        insts = [_scan(s, scans[s][1], seed=k) for k, s in enumerate(ids)]
        c[name] = dict(kind='pred', args=(ids, insts, nyu), tiny=tiny)
    gt_ids = ['scene0000_00', 'scene0011_01']
    gts = [_gt_ids(21, 3001), _gt_ids(22, 2048)]
    c['gt_scannet'] = dict(kind='gt', args=(gt_ids, gts, NYU_ID), tiny=False)
    c['gt_plain'] = dict(kind='gt', args=(gt_ids, gts, None), tiny=False)
    c['gt_tiny'] = dict(kind='gt', args=(['t'], [np.array([0, 1000, 1999, 18000, 18999, 7, 0], np.int64)], NYU_ID),
                        tiny=True)
    c['lines'] = dict(kind='gt', args=(['powers', 'empty'], [_powers(), np.zeros(0, np.int64)], None), tiny=True)
    frames = ['sequences/08/velodyne/000123', 'sequences/08/velodyne/000124']
    c['panoptic'] = dict(kind='panoptic', args=(frames, [_kitti_words(31, 3001), _kitti_words(32, 2500)],
                                                LEARNING_MAP_INV, KITTI_CLASSES), tiny=False)
    c['panoptic_tiny'] = dict(kind='panoptic', args=(['sequences/11/velodyne/000000'], [_kitti_words(33, 23)],
                                                     LEARNING_MAP_INV, KITTI_CLASSES), tiny=True)
    bad = _kitti_words(34, 500)
    bad[137] = np.uint32(20 | (5 << 16))
    c['panoptic_unmapped'] = dict(kind='panoptic', args=(['sequences/08/velodyne/000200'], [bad], LEARNING_MAP_INV,
                                                         KITTI_CLASSES), tiny=False, raises='KeyError')
    sem_ids = ['scene0000_00', 'Area_5_office_1']
    arrs = [_semantic_arrays(41, 257), _semantic_arrays(42, 100)]
    c['npy'] = dict(kind='npy', args=(sem_ids, {k: [a[k] for a in arrs] for k in arrs[0]}), tiny=False)
    return c
