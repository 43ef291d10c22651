"""Deterministic result trees for the visualization golden (visualization_golden.json, written by
make_visualization_golden.py from the reference's tools/visualization.py).  numpy only.

cases(): name -> dict with
    room             the scan id
    n                points
    coords, colors, offset_pred   float32 [n, 3]
    semantic_label, semantic_pred int64 [n]
    gt_ids           int64 [n]: class * 1000 + instance + 1, 0 = ignore (what save_gt_instances writes)
    insts            [(label id, score, uint8 mask [n])]: pred_instance/<room>.txt and its mask files
    remove           relative paths deleted from the tree after it is written (the missing-file cases)
    tiny             True: the golden stores the PLY bytes, not only size and SHA-256
    errors           {task: exception name} the reference raises and the project must raise too
    instead          {task: 'empty' | 'printf'}: the reference fails inside itemgetter on a degenerate scan (no
                     labelled point; a single point); the project writes the cloud the other tasks show -- no
                     vertex at all / the one vertex, which the test prints with '%f' itself
    declines         tasks ('all' or a set) whose file the device kernels leave to the numpy path
write_tree(case, root): the tree as softgroup_amd.util.save_results lays it out.

In every case the populations of the drawn masks are pairwise distinct, so are the sizes of the ground-truth
instances and so are the scores: the reference's unstable argsort then has no ties to break (check_distinct).
"""
import os

import numpy as np

TASKS = ('input', 'semantic_gt', 'semantic_pred', 'offset_semantic_pred', 'instance_gt', 'instance_pred')
F32 = np.float32


def _base(room, n, seed, tiny=False):
    rng = np.random.default_rng(seed)
    f3 = lambda s: (rng.standard_normal((n, 3)) * s).astype(F32)  # noqa: E731
    label = rng.integers(0, 20, size=n)
    label[rng.random(n) < 0.15] = -100
    return dict(room=room, n=n, coords=f3(3.0), colors=rng.uniform(-1, 1, size=(n, 3)).astype(F32),
                offset_pred=f3(0.1), semantic_label=label.astype(np.int64),
                semantic_pred=rng.integers(0, 20, size=n).astype(np.int64), gt_ids=np.zeros(n, np.int64), insts=[],
                remove=[], tiny=tiny, errors={}, instead={}, declines=set())


def _gt_by_sizes(n, sizes, seed):
    """instance k (0-based) gets sizes[k] points, scattered; the rest is ignore (0)"""
    rng = np.random.default_rng(seed)
    ids = np.zeros(n, np.int64)
    where = rng.permutation(n)[:sum(sizes)]
    at = 0
    for k, s in enumerate(sizes):
        ids[where[at:at + s]] = (k % 18 + 1) * 1000 + k + 1
        at += s
    return ids


def _masks_by_sizes(n, sizes, seed, overlap=True):
    """mask k is a window of sizes[k] consecutive points; the windows overlap freely"""
    rng = np.random.default_rng(seed)
    out = []
    for s in sizes:
        lo = int(rng.integers(0, n - s + 1)) if overlap else 0
        m = np.zeros(n, np.uint8)
        m[lo:lo + s] = 1
        out.append(m)
    return out


def _scores(k, seed, low=()):
    """k pairwise distinct scores with four decimals; the entries of `low` are under the 0.09 cut"""
    rng = np.random.default_rng(seed)
    s = (rng.permutation(9000)[:k] + 900) / 10000.0
    for j, i in enumerate(low):
        s[i] = (j + 1) / 1000.0
    return [float(x) for x in s]


def _room():
    c = _base('scene0011_00', 3001, 1)
    c['semantic_label'][5:9] = -1                                   # kept, and black under semantic_gt
    c['gt_ids'] = _gt_by_sizes(c['n'], [300, 7, 150, 1, 90, 420, 33, 2, 260], 2)
    free = np.flatnonzero(c['gt_ids'] == 0)[:3]
    c['gt_ids'][free] = [2000, 18000, 1000]                         # % 1000 - 1 == -1, like 0: instance of no colour
    sizes = [500, 40, 333, 1200, 64, 7, 250, 800, 128, 90, 2000, 31]
    masks = _masks_by_sizes(c['n'], sizes, 3)
    scores = _scores(len(sizes), 4, low=(1, 10))                    # two masks under the cut, one of them the largest
    c['insts'] = [(k % 18 + 1, scores[k], masks[k]) for k in range(len(sizes))]
    return c


def _wrap():
    c = _base('scene0704_01', 4000, 5)
    c['gt_ids'] = _gt_by_sizes(c['n'], list(range(1, 71)), 6)       # 70 instances: the 68-colour palette wraps
    sizes = list(range(30, 105))                                    # 75 masks
    masks = _masks_by_sizes(c['n'], sizes, 7)
    scores = _scores(len(sizes), 8, low=(3, ))
    c['insts'] = [(k % 18 + 1, scores[k], masks[k]) for k in range(len(sizes))]
    return c


def formatter_values():
    """float32 values for the '%f' formatter, all below 2^31 in magnitude"""
    v = [-0.0, 0.0, -1e-9, 1e-9, 0.5e-6, 1.5e-6, 2.5e-6, -0.5e-6, -1.5e-6, 0.1, 0.999999, 0.9999995, 9.9999995,
         99999.9999995, 123456.789, -123456.789, 1e-45, -1e-40, 1.1754942e-38, 1.17549435e-38, 16777216.0, 1e9,
         2147483520.0, -2147483520.0, 1073741824.0, 0.3, 2.0 / 3.0, 1e-6, 1e-7, 4.9999999e-7, 5.0000001e-7]
    v += [j / 128.0 for j in (1, 3, 5, 7, 129, -1, -3, 255)]       # exact ties at the sixth decimal: half to even
    out = []
    for x in v:
        x = F32(x)
        out += [np.nextafter(x, F32(-np.inf), dtype=F32), x, np.nextafter(x, F32(np.inf), dtype=F32)]
    out = [x for x in out if abs(float(x)) < 2.0**31]
    while len(out) % 3:
        out.append(F32(0.25))
    return np.array(out, dtype=F32)


def _small(room, n, seed, **kw):
    c = _base(room, n, seed, tiny=True)
    c['semantic_label'][:] = np.arange(n) % 20
    c['gt_ids'] = _gt_by_sizes(n, [s for s in (3, 1, 2) if s <= n // 2] or [1], seed + 50)
    sizes = [s for s in (n, max(n // 2, 1) if n > 1 else 0, 1 if n > 3 else 0) if s]
    sizes = sorted(set(sizes), reverse=True)
    masks = _masks_by_sizes(n, sizes, seed + 60)
    scores = _scores(len(sizes), seed + 70)
    c['insts'] = [(k + 1, scores[k], masks[k]) for k in range(len(sizes))]
    c.update(kw)
    return c


def _formatter():
    v = formatter_values().reshape(-1, 3)
    c = _small('formatter', len(v), 9)
    c['coords'] = v.copy()
    c['offset_pred'][:] = 0
    c['offset_pred'][::2] = F32(1e-7)
    return c


def _huge():
    c = _small('huge', 6, 10, declines='all')
    c['coords'][0] = [2.0**31, 1.0, -1.0]
    c['coords'][3] = [-2.0**31, 3e9, 1e38]
    return c


def _nonfinite():
    c = _small('nonfinite', 6, 11, declines='all')
    c['coords'][1] = [np.inf, -np.inf, np.nan]
    c['offset_pred'][:] = 0
    return c


def _colour_range():
    c = _small('colour_range', 8, 12, declines={'input'})
    c['colors'][0] = [1.5, -1.3, 1.0]
    c['colors'][1] = [-1.0, 1.004, -1.004]
    return c


def _all_filtered():
    c = _small('all_filtered', 7, 13, instead={'semantic_gt': 'empty'})
    c['semantic_label'][:] = -100
    return c


def _single_kept():
    c = _small('single_kept', 5, 14)
    c['semantic_label'][:] = -100
    c['semantic_label'][2] = 3
    return c


def _one_point():
    c = _small('one_point', 1, 15, instead={'semantic_pred': 'printf', 'offset_semantic_pred': 'printf'})
    c['coords'][0] = [-0.0, 1.5e-6, 123456.789]
    c['offset_pred'][0] = [0.5, 0.0, 0.25]
    c['semantic_label'][0] = 7
    c['semantic_pred'][0] = 3
    return c


def _class20():
    c = _small('class20', 10, 16, errors={'semantic_gt': 'IndexError', 'semantic_pred': 'IndexError',
                                          'offset_semantic_pred': 'IndexError'})
    c['semantic_label'][4] = 20
    c['semantic_pred'][6] = 20
    return c


def _missing_pred():
    c = _small('missing_pred', 9, 17, errors={'semantic_pred': 'AssertionError', 'offset_semantic_pred': 'AssertionError',
                                              'instance_pred': 'AssertionError'})
    c['remove'] = ['semantic_pred/missing_pred.npy', 'pred_instance/missing_pred.txt']
    return c


def _missing_mask():
    c = _small('missing_mask', 9, 18, errors={'offset_semantic_pred': 'AssertionError', 'instance_pred': 'AssertionError'})
    c['remove'] = ['offset_pred/missing_mask.npy', 'pred_instance/predicted_masks/missing_mask_001.txt']
    return c


def _missing_coords():
    c = _small('missing_coords', 9, 19, errors={t: 'FileNotFoundError' for t in TASKS})
    c['remove'] = ['coords/missing_coords.npy']
    return c


def cases():
    built = [_room(), _wrap(), _formatter(), _huge(), _nonfinite(), _colour_range(), _all_filtered(), _single_kept(),
             _one_point(), _class20(), _missing_pred(), _missing_mask(), _missing_coords()]
    return {c['room']: c for c in built}


def check_distinct(case):
    """the condition under which the reference's output does not depend on its sort's tie order"""
    scores = [format(s, '.4f') for _, s, _ in case['insts']]
    assert len(set(scores)) == len(scores), case['room']
    drawn = [int(m.sum()) for _, s, m in case['insts'] if float(format(s, '.4f')) >= 0.09]
    drawn = [p for p in drawn if p]
    assert len(set(drawn)) == len(drawn), case['room']
    label = case['gt_ids'] % 1000 - 1
    sizes = np.bincount(label[label >= 0]) if (label >= 0).any() else np.zeros(0, int)
    sizes = sizes[sizes > 0]
    assert len(set(sizes.tolist())) == len(sizes), case['room']


def mask_name(room, k):
    return 'predicted_masks/%s_%03d.txt' % (room, k)


def write_tree(case, root):
    room = case['room']
    for directory in ('coords', 'colors', 'semantic_label', 'semantic_pred', 'offset_pred', 'gt_instance',
                      'pred_instance/predicted_masks'):
        os.makedirs(os.path.join(root, directory), exist_ok=True)
    for directory in ('coords', 'colors', 'semantic_label', 'semantic_pred', 'offset_pred'):
        np.save(os.path.join(root, directory, room + '.npy'), case[directory])
    with open(os.path.join(root, 'gt_instance', room + '.txt'), 'w') as f:
        f.write(''.join('%d\n' % v for v in case['gt_ids'].tolist()))
    lines = []
    for k, (label, score, mask) in enumerate(case['insts']):
        lines.append('%s %d %s\n' % (mask_name(room, k), label, format(score, '.4f')))
        with open(os.path.join(root, 'pred_instance', mask_name(room, k)), 'w') as f:
            f.write(''.join('%d\n' % v for v in mask.tolist()))
    with open(os.path.join(root, 'pred_instance', room + '.txt'), 'w') as f:
        f.write(''.join(lines))
    for rel in case['remove']:
        os.remove(os.path.join(root, rel))
