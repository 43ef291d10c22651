"""Coloured point clouds of a test run: what the reference's tools/visualization.py makes of an ``--out``
directory (``get_coords_color`` :141-231, ``write_ply`` :234-260) for its six tasks -- ``input``,
``semantic_gt``, ``semantic_pred``, ``offset_semantic_pred``, ``instance_gt``, ``instance_pred`` -- with the PLY
files byte for byte.  It reads the tree ``softgroup_amd.util.save_results`` writes, or takes the result dicts of
``forward_test`` directly (``colors_from_result``).

The reference reads every predicted mask with ``splitlines``, paints with one full-array comparison per
instance and prints one ``str.format`` per vertex.  Here:

  * ``backend='device'``: viz_io.hip.  The mask files are parsed straight into bit rows (sg_parse_mask_text),
    sg_viz_paint_bits / sg_viz_paint_runs paint, sg_viz_gt_labels and sg_viz_instance_rank order the instances,
    sg_viz_colors looks the colours up and sg_viz_ply_vertices prints the vertex lines into a device buffer;
    one copy to pinned memory, and a thread pool writes the files from there.  What the kernels decline -- a
    coordinate that is not finite or is 2^31 or more in magnitude, an ``input`` colour outside 0..255 -- is
    formatted by the numpy path, with the same bytes; the dict returned per file says who formatted it.
  * ``backend='numpy'``: the same bytes from vectorised numpy (integer arithmetic on the float32 bit patterns,
    no per-vertex Python), for tooling without a GPU.  float64 vertices, faces and the declined rows above go
    through ``np.char.mod`` under every backend.
  * ``backend='auto'``: numpy without a GPU; with one, ``_AUTO`` below per kind of work (``paint`` = labels,
    colours and PLY text, ``read`` = the mask and id files).  tools/visualization_bench.py is the measurement
    that decides it; no table of it is recorded, so both kinds are on numpy and ``'device'`` is asked for by
    name.

Instance order.  The reference orders instances with ``np.argsort(...)[::-1]`` twice: by score for the paint
priority of ``instance_pred`` and by point count for the palette.  That sort is not stable, so equal keys come
out differently on different numpy builds.  The rule here, on every backend: descending key, and among equal
keys the HIGHER index first (a stable ascending sort read backwards).  Ids without points take the last ranks
and paint nothing.

What differs from the reference, on purpose:
  * ``get_coords_color`` returns, for the two instance tasks, the palette's integers (as float64) where the
    reference returns the float32 product ``table * 255`` (113.985 for 113): the palettes are kept as the uint8
    values write_ply prints.  ``int(rgb / 255 * 255)`` is the same integer either way.
  * a scan without a single labelled point (``semantic_gt``) and a scan of one point (``semantic_pred``) end in a
    TypeError / IndexError inside ``itemgetter`` in the reference; here they give the cloud the other tasks give.
"""
import os
import os.path as osp
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from ..ops._args import choose_backend
from .results import _POW10, _THREADS, _Stage, _Writer, _host, _read_bytes, _runs_of, read_int_lines, read_mask

__all__ = ['TASKS', 'INSTANCE_PALETTE', 'SCANNET_CLASS_PALETTE', 'get_coords_color', 'colors_from_result',
           'write_ply', 'save_visualizations']

TASKS = ('input', 'semantic_gt', 'semantic_pred', 'offset_semantic_pred', 'instance_gt', 'instance_pred')
# what 'auto' means with a GPU present (module docstring)
_AUTO = {'paint': 'numpy', 'read': 'numpy'}
_SCORE_CUT = 0.09              # masks below it are not drawn (visualization.py:215)
_GT_IDS = 999                  # ids % 1000 - 1 lies in -1 .. 998
_NONE = -100                   # label of an unpainted point, and the semantic label that drops a point
_MODE = {'input': 0, 'semantic_gt': 1, 'semantic_pred': 2, 'offset_semantic_pred': 2, 'instance_gt': 3,
         'instance_pred': 3}   # softgroup_hip.h: SG_VIZ_*


def _table(hex_rows):
    t = np.frombuffer(bytes.fromhex(''.join(hex_rows)), dtype=np.uint8).reshape(-1, 3).copy()
    t.setflags(write=False)
    return t


# The 68 instance colours as write_ply prints them, RRGGBB per row.
INSTANCE_PALETTE = _table((
    '0071bc', 'd85218', 'ecb01f', '7d2e8d', '76ab2f', '4cbded', 'a1132e', '999999', 'ff0000', 'ff7f00', 'bebe00',
    '00ff00', '0000ff', 'aa00ff', '545400', '54aa00', '54ff00', 'aa5400', 'aaaa00', 'aaff00', 'ff5400', 'ffaa00',
    'ffff00', '00547f', '00aa7f', '00ff7f', '54007f', '54547f', '54aa7f', '54ff7f', 'aa007f', 'aa547f', 'aaaa7f',
    'aaff7f', 'ff007f', 'ff547f', 'ffaa7f', 'ffff7f', '0054ff', '00aaff', '00ffff', '5400ff', '5454ff', '54aaff',
    '54ffff', 'aa00ff', 'aa54ff', 'aaaaff', 'aaffff', 'ff00ff', 'ff54ff', 'ffaaff', '7f0000', 'aa0000', 'd40000',
    'ff0000', '002a00', '007f00', '00aa00', '00d400', '00ff00', '00002a', '00007f', '0000aa', '0000d4', '0000ff',
    '242424', 'dadada'))
# The ScanNet benchmark's colour of the 20 evaluated classes, by class id: wall, floor, cabinet, bed, chair, sofa,
# table, door, window, bookshelf, picture, counter, desk, curtain, refrigerator, shower curtain, toilet, sink,
# bathtub, other furniture.
SCANNET_CLASS_PALETTE = _table((
    'abc6e6', '8fdf8e', '0078b1', 'ffbc7e', 'bdbd39', '90564c', 'ff9899', 'de282f', 'c5b0d4', '9667b9', 'c89c95',
    '00bece', 'fcb7d2', 'dbdb92', 'ff7f2b', '96dae4', '00a037', '6e808f', 'ea77c0', '5053a0'))

_HEADER = ('ply \nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n'
           'property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\n'
           'property list uchar uint vertex_indices\nend_header\n')


def _choose(backend, kind):
    return choose_backend(backend, _AUTO[kind])


def _palette(table, default):
    if table is None:
        return default
    table = np.ascontiguousarray(table)
    if table.ndim != 2 or table.shape[1] != 3 or table.shape[0] == 0 or table.dtype.kind not in 'iu' or \
            table.min() < 0 or table.max() > 255:
        raise ValueError('a palette is an integer table [k, 3] of values 0..255')
    return table.astype(np.uint8)


# ---- the inputs of one scan ------------------------------------------------------------------------------------
class _Scan:
    """the inputs of one scan: every entry is produced on first use and shared by the tasks"""

    def __init__(self, getters):
        self.getters, self.cache = getters, {}

    def __getitem__(self, key):
        if key not in self.cache:
            self.cache[key] = self.getters[key]()
        return self.cache[key]


def _load_npy(path, message=None):
    if message is not None:
        assert osp.isfile(path), message.format(path)
    elif not osp.isfile(path):
        raise FileNotFoundError(f'No such file: {path}')
    return np.load(path)


def _dense_to_bits(masks, n):
    words = (n + 31) // 32
    padded = np.zeros((len(masks), words * 32), dtype=np.uint8)
    for k, m in enumerate(masks):
        if m is not None:
            padded[k, :n] = m
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder='little')).view(np.int32).reshape(-1, words)


def _checked_mask(path, n, backend):
    m = read_mask(path, backend)
    if m.size != n:
        raise ValueError(f'{path}: a mask of {m.size} points for a scan of {n}')
    return m


def _file_instances(root, room, n, read_backend, stage):
    """scores, skip flags and masks of pred_instance/<room>.txt.  masks: ('dense', [bool array | None]) or, read
    on the device, ('bits', int32 tensor [n_inst, ceil(n / 32)]); the masks under the score cut are not read.
    reparsed: mask files the device parser declined (not '0' | '1' and a newline per point) and numpy read."""
    summary = osp.join(root, 'pred_instance', room + '.txt')
    assert osp.isfile(summary), 'No instance result - {}.'.format(summary)
    with open(summary) as f:
        fields = [line.rstrip().split() for line in f.readlines()]
    scores = np.array([float(x[-1]) for x in fields], dtype=np.float64)
    paths = [osp.join(root, 'pred_instance', x[0]) for x in fields]
    for p in paths:
        assert osp.isfile(p), p
    skip = np.array([float(x[2]) < _SCORE_CUT for x in fields], dtype=bool)
    drawn = [k for k in range(len(paths)) if not skip[k]]
    if read_backend != 'device' or stage is None or n == 0:
        masks = [None] * len(paths)
        for k in drawn:
            masks[k] = _checked_mask(paths[k], n, 'numpy' if read_backend != 'device' else read_backend)
        return dict(scores=scores, skip=skip, masks=('dense', masks), reparsed=0)
    torch, L, lib = stage.torch, stage.L, stage.lib
    words = (n + 31) // 32
    bits = torch.zeros((len(paths), words), dtype=torch.int32, device=stage.dev)
    metas = torch.zeros((max(len(paths), 1), 2), dtype=torch.int64, device=stage.dev)
    with ThreadPoolExecutor(max_workers=_THREADS) as pool:
        texts = list(pool.map(_read_bytes, [paths[k] for k in drawn]))
    redo = []
    for k, data in zip(drawn, texts):
        if len(data) not in (2 * n - 1, 2 * n) or len(data) >= 2**32:      # (a row holds exactly ceil(n / 32) words)
            redo.append(k)
            continue
        text = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(stage.dev)
        L.check(lib.sg_parse_mask_text(L.ptr(text), len(data), None, bits.data_ptr() + 4 * k * words,
                                       metas.data_ptr() + 16 * k, L.stream()), 'sg_parse_mask_text')
    bad = metas[:, 1].cpu().numpy()
    redo += [k for k in drawn if bad[k] and k not in redo]
    for k in redo:                                                           # hand-written files
        row = _dense_to_bits([_checked_mask(paths[k], n, 'numpy')], n)
        bits[k].copy_(torch.from_numpy(row[0]))
    return dict(scores=scores, skip=skip, masks=('bits', bits), reparsed=len(redo))


def _file_scan(prediction_path, room, read_backend, stage=None):
    root = prediction_path

    def path(directory, ext='.npy'):
        return osp.join(root, directory, room + ext)

    for directory, ext in (('coords', '.npy'), ('colors', '.npy'), ('semantic_label', '.npy'), ('gt_instance', '.txt')):
        if not osp.isfile(path(directory, ext)):                             # the reference opens all four for every task
            raise FileNotFoundError(f'No such file: {path(directory, ext)}')
    scan = _Scan({})
    scan.getters.update(
        coords=lambda: _load_npy(path('coords')),
        colors=lambda: _load_npy(path('colors')),
        semantic_label=lambda: _load_npy(path('semantic_label')),
        gt_ids=lambda: read_int_lines(path('gt_instance', '.txt'), read_backend),
        semantic_pred=lambda: _load_npy(path('semantic_pred'), 'No semantic result - {}.'),
        offset_pred=lambda: _load_npy(path('offset_pred'), 'No offset result - {}.'),
        instances=lambda: _file_instances(root, room, len(scan['coords']), read_backend, stage))
    return scan


def _result_scan(result):
    def instances():
        insts = list(result['pred_instances'])
        # the summary file carries the confidence to four decimals; the cut and the order see that value
        scores = np.array([float(format(i['conf'], '.4f')) for i in insts], dtype=np.float64)
        runs = [_runs_of(i['pred_mask']) for i in insts]
        n = len(_host(result['coords_float']))
        for length, _, _ in runs:
            if length != n:
                raise ValueError(f'a mask of {length} points for a scan of {n}')
        return dict(scores=scores, skip=scores < _SCORE_CUT, masks=('runs', runs))

    return _Scan(dict(
        coords=lambda: _host(result['coords_float']), colors=lambda: _host(result['color_feats']),
        semantic_label=lambda: _host(result['semantic_labels']),
        gt_ids=lambda: _host(result['gt_instances']).reshape(-1).astype(np.int64),
        semantic_pred=lambda: _host(result['semantic_preds']), offset_pred=lambda: _host(result['offset_preds']),
        instances=instances))


# ---- order ---------------------------------------------------------------------------------------------------------
def _ascending_position(keys):
    """position of every entry in a stable ascending sort"""
    order = np.argsort(keys, kind='stable')
    pos = np.empty(len(order), dtype=np.int32)
    pos[order] = np.arange(len(order), dtype=np.int32)
    return pos


def _rank(pointnum):
    """the module's rule: position by descending count, the higher index first among equal counts"""
    return (len(pointnum) - 1 - _ascending_position(pointnum)).astype(np.int32)


# ---- numpy path ------------------------------------------------------------------------------------------------
def _dense(mask_kind, mask, n):
    if mask_kind == 'dense':
        return mask
    _, starts, ends = mask
    step = np.zeros(n + 1, dtype=np.int8)
    step[starts] += 1
    step[ends] -= 1
    return np.cumsum(step[:-1], dtype=np.int8) > 0


def _paint_numpy(n, inst):
    kind, masks = inst['masks']
    if kind == 'bits':
        bits = masks.cpu().numpy().view(np.uint32)
        rows = np.unpackbits(bits.view(np.uint8), axis=1, bitorder='little')[:, :n].astype(bool)
        kind, masks = 'dense', list(rows)
    label = np.full(n, _NONE, dtype=np.int64)
    pointnum = np.zeros(len(masks), dtype=np.int64)
    for k in np.argsort(inst['scores'], kind='stable'):          # ascending priority: the last write wins
        if inst['skip'][k]:
            continue
        m = _dense(kind, masks[k], n)
        pointnum[k] = m.sum()
        label[m] = k
    return label, pointnum


def _lookup(table, label, rank=None):
    rgb = np.zeros((len(label), 3), dtype=np.float64)
    sel = label >= 0
    idx = label[sel]
    if rank is not None:
        idx = rank[idx] % len(table)
    elif idx.size and idx.max() >= len(table):
        raise IndexError(f'index {int(idx.max())} is out of bounds for a palette of {len(table)} classes')
    rgb[sel] = table[idx]
    return rgb


def _rgb_numpy(scan, task, inst_table, class_table):
    """``rgb`` as get_coords_color returns it, before the filter"""
    rgb = (scan['colors'] + 1) * 127.5
    n = len(rgb)
    if task == 'semantic_gt':
        rgb = _lookup(class_table, scan['semantic_label'].astype(np.int64))
    elif task in ('semantic_pred', 'offset_semantic_pred'):
        rgb = class_table.astype(np.int64)[scan['semantic_pred'].astype(np.int64)].reshape(n, 3)
    elif task == 'instance_gt':
        label = scan['gt_ids'] % 1000 - 1
        rgb = _lookup(inst_table, label, _rank(np.bincount(label[label >= 0], minlength=_GT_IDS)))
    elif task == 'instance_pred':
        label, pointnum = _paint_numpy(n, scan['instances'])
        rgb = _lookup(inst_table, label, _rank(pointnum))
    return rgb


def _xyz(scan, task):
    xyz = scan['coords']
    if task == 'offset_semantic_pred':
        xyz = xyz + scan['offset_pred']
    return xyz


def _printed(colors):
    """``int(c * 255)`` per component (visualization.py:255-257) as int64; raises what ``int`` raises"""
    v = np.asarray(colors) * 255
    if v.dtype.kind == 'f':
        if np.isnan(v).any():
            raise ValueError('cannot convert float NaN to integer')
        if np.isinf(v).any():
            raise OverflowError('cannot convert float infinity to integer')
        v = np.trunc(v)
    return v.astype(np.int64)


def _fixed6(x):
    """float32 [..] -> (sign bit, round-half-even(|x| * 10^6) as uint64, accepted): integer arithmetic on the bit
    pattern, as viz_io.hip's viz_fixed6.  Not accepted: not finite, or 2^31 and above."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    e = ((b >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int64)
    m = (b & np.uint32(0x7FFFFF)).astype(np.uint64)
    ok = e < 158
    p = np.where(e == 0, m, m | np.uint64(0x800000)) * np.uint64(10**6)
    s = np.where(e == 0, 149, 150 - e)
    left = np.clip(-s, 0, 7).astype(np.uint64)
    right = np.clip(s, 1, 63).astype(np.uint64)                  # (from 2^-44 down everything rounds to 0)
    q = p >> right
    r = p & ((np.uint64(1) << right) - np.uint64(1))
    half = np.uint64(1) << (right - np.uint64(1))
    q = q + ((r > half) | ((r == half) & ((q & np.uint64(1)) == 1))).astype(np.uint64)
    q = np.where(s <= 0, p << left, np.where(s >= 64, np.uint64(0), q))
    return (b >> np.uint32(31)).astype(bool), q, ok


def _digits(v):
    return np.searchsorted(_POW10, v, side='right') + 1


def _put_digits(out, last, value, count):
    """decimal digits of value, `count` of them, the last one at out[last]"""
    for k in range(int(count.max()) if count.size else 0):
        sel = count > k
        out[last[sel] - k] = (value[sel] // np.uint64(10**k) % np.uint64(10)).astype(np.uint8) + 48


def _vertex_text_numpy(xyz, ints):
    """the vertex lines of write_ply for xyz [m, 3] and printed colours int64 [m, 3], as a uint8 array"""
    m = len(xyz)
    if m == 0:
        return np.empty(0, dtype=np.uint8)
    xyz = np.asarray(xyz)[:, :3]
    ok = None
    if xyz.dtype == np.float32:
        neg_f, q, ok = _fixed6(xyz)
    if ok is None or not ok.all():
        # float64 vertices, and what the integer path declines: one C-level pass of Python's own '%f' / '%d'
        cols = [np.char.mod('%f', xyz[:, c].astype(np.float64)) for c in range(3)]
        cols += [np.char.mod('%d', ints[:, c]) for c in range(3)]
        line = cols[0]
        for c in cols[1:]:
            line = np.char.add(np.char.add(line, ' '), c)
        return np.frombuffer(('\n'.join(line.tolist()) + '\n').encode(), dtype=np.uint8)
    ip, fr = q // np.uint64(10**6), q % np.uint64(10**6)
    neg_c = ints < 0
    mag_c = np.where(neg_c, -ints, ints).astype(np.uint64)
    nd_f, nd_c = _digits(ip), _digits(mag_c)
    width = np.concatenate([neg_f + nd_f + 7, neg_c + nd_c], axis=1) + 1
    end = np.cumsum(width.reshape(-1)).reshape(m, 6)
    start = end - width
    out = np.empty(int(end[-1, -1]), dtype=np.uint8)
    out[end[:, :5] - 1] = 32
    out[end[:, 5] - 1] = 10
    ef, ec = end[:, :3], end[:, 3:]
    _put_digits(out, ef - 2, fr, np.full(fr.shape, 6))
    out[ef - 8] = 46
    _put_digits(out, ef - 9, ip, nd_f)
    out[start[:, :3][neg_f]] = 45
    _put_digits(out, ec - 2, mag_c, nd_c)
    out[start[:, 3:][neg_c]] = 45
    return out


def _face_text(indices):
    if indices is None or len(indices) == 0:
        return b''
    idx = np.asarray(indices)
    if idx.dtype.kind not in 'iu':
        raise ValueError(f"Unknown format code 'd' for object of type '{idx.dtype}'")
    return ''.join('3 %d %d %d\n' % (a, b, c) for a, b, c in idx[:, :3].tolist()).encode()


def _write_parts(path, parts):
    with open(path, 'wb') as f:
        for p in parts:
            f.write(p)


# ---- device path -------------------------------------------------------------------------------------------------
def _labels_device(stage, scan, task, n):
    """(int32 labels, int32 ranks) on the device for the two instance tasks"""
    torch, L, lib = stage.torch, stage.L, stage.lib
    label = torch.empty(max(n, 1), dtype=torch.int32, device=stage.dev)
    if task == 'instance_gt':
        n_inst = _GT_IDS
        pointnum = torch.empty(n_inst, dtype=torch.int32, device=stage.dev)
        ids = stage.upload(scan['gt_ids'], np.int64)
        L.check(lib.sg_viz_gt_labels(L.ptr(ids), n, L.ptr(label), L.ptr(pointnum), L.stream()), 'sg_viz_gt_labels')
    else:
        inst = scan['instances']
        n_inst = len(inst['scores'])
        pointnum = torch.empty(max(n_inst, 1), dtype=torch.int32, device=stage.dev)
        priority = stage.upload(_ascending_position(inst['scores']), np.int32)
        skip = stage.upload(inst['skip'], np.uint8)
        kind, masks = inst['masks']
        if kind == 'runs':
            bounds = np.zeros(n_inst + 1, dtype=np.int64)
            np.cumsum([r[1].size for r in masks], out=bounds[1:])
            cat = (lambda j: np.concatenate([r[j] for r in masks])) if masks else (lambda j: np.zeros(0, np.int64))
            starts, ends = stage.upload(cat(1), np.int32), stage.upload(cat(2), np.int32)
            bounds_d = stage.upload(bounds, np.int64)
            ws = L.workspace(lib.sg_viz_paint_runs_workspace_bytes(n_inst, n), stage.dev)
            L.check(lib.sg_viz_paint_runs(L.ptr(starts), L.ptr(ends), L.ptr(bounds_d), int(bounds[-1]), n_inst, n,
                                          L.ptr(priority), L.ptr(skip), L.ptr(label), L.ptr(pointnum), L.ptr(ws),
                                          ws.numel(), L.stream()), 'sg_viz_paint_runs')
        else:
            bits = masks if kind == 'bits' else stage.upload(_dense_to_bits(masks, n), np.int32)
            L.check(lib.sg_viz_paint_bits(L.ptr(bits), n_inst, n, L.ptr(priority), L.ptr(skip), L.ptr(label),
                                          L.ptr(pointnum), L.stream()), 'sg_viz_paint_bits')
    rank = torch.empty(max(n_inst, 1), dtype=torch.int32, device=stage.dev)
    ws = L.workspace(lib.sg_viz_instance_rank_workspace_bytes(n_inst), stage.dev)
    L.check(lib.sg_viz_instance_rank(L.ptr(pointnum), n_inst, L.ptr(rank), L.ptr(ws), ws.numel(), L.stream()),
            'sg_viz_instance_rank')
    return label, rank, n_inst


def _rgb_device(stage, scan, task, inst_table, class_table):
    """(uint8 [n, 3] device tensor of the printed colours, colour components a uint8 cannot hold)"""
    torch, L, lib = stage.torch, stage.L, stage.lib
    mode = _MODE[task]
    n = len(scan['coords'])
    rgb = torch.empty((max(n, 1), 3), dtype=torch.uint8, device=stage.dev)
    colors = cls = label = rank = table = None
    n_rank = 0
    if mode == 0:
        colors = stage.upload(scan['colors'], np.float32)
    elif mode == 3:
        label, rank, n_rank = _labels_device(stage, scan, task, n)
        table = stage.upload(inst_table, np.uint8)
    else:
        cls = stage.upload(scan['semantic_label' if task == 'semantic_gt' else 'semantic_pred'], np.int64)
        table = stage.upload(class_table, np.uint8)
    L.check(lib.sg_viz_colors(mode, L.ptr(colors), L.ptr(cls), L.ptr(label), L.ptr(rank), n_rank, L.ptr(table),
                              0 if table is None else table.shape[0], n, L.ptr(rgb), L.ptr(stage.meta), L.stream()),
            'sg_viz_colors')
    bad, nan, wide = stage.meta[:3].cpu().tolist()
    if bad:
        raise IndexError(f'{bad} labels out of bounds for a palette of {table.shape[0]} rows')
    if nan:
        raise ValueError('cannot convert float NaN to integer')
    return rgb[:n], wide


def _vertex_text_device(stage, xyz, offset, rgb, keep, n):
    """sg_viz_ply_vertices -> (pinned tensor, futures list of that buffer, bytes, vertices, declined rows)"""
    L, lib = stage.L, stage.lib
    cap = 69 * n
    text, pinned, busy = stage.take(cap)
    ws = stage.workspace(lib.sg_viz_ply_vertices_workspace_bytes(n))
    L.check(lib.sg_viz_ply_vertices(L.ptr(xyz), L.ptr(offset), L.ptr(rgb), L.ptr(keep), n, L.ptr(text), cap,
                                    L.ptr(stage.meta), L.ptr(ws), ws.numel(), L.stream()), 'sg_viz_ply_vertices')
    total, kept, declined, dropped = stage.meta[:4].cpu().tolist()
    assert dropped == 0, 'sg_viz_ply_vertices: text bound too small'
    return pinned, busy, total, kept, declined


# ---- one cloud ---------------------------------------------------------------------------------------------------
def _cloud_numpy(scan, task, inst_table, class_table):
    """(xyz, rgb) of the reference's get_coords_color, filtered"""
    rgb = _rgb_numpy(scan, task, inst_table, class_table)
    keep = scan['semantic_label'] != _NONE
    return _xyz(scan, task)[keep], rgb[keep]


def _cloud_file(w, stage, scan, task, path, inst_table, class_table):
    """writes the task's PLY; the description of the file.  stage None: numpy."""
    info = dict(path=path, task=task, formatted_by='numpy', declined=0)
    if task == 'instance_pred':
        info['masks_reparsed'] = scan['instances'].get('reparsed', 0)
    if stage is not None:
        n = len(scan['coords'])
        rgb, wide = _rgb_device(stage, scan, task, inst_table, class_table)
        info['declined'] = wide
        if not wide and n:
            xyz = stage.upload(scan['coords'], np.float32)
            offset = stage.upload(scan['offset_pred'], np.float32) if task == 'offset_semantic_pred' else None
            keep = stage.upload(scan['semantic_label'] != _NONE, np.uint8)
            pinned, busy, total, kept, declined = _vertex_text_device(stage, xyz, offset, rgb, keep, n)
            info['declined'] = declined
            if not declined:
                host = stage.to_host(pinned, total)
                busy.append(w.call(_write_parts, path, ((_HEADER % (kept, 0)).encode(), host[:total])))
                info.update(formatted_by='device', vertices=kept, bytes=len(_HEADER % (kept, 0)) + total)
                return info
    xyz, rgb = _cloud_numpy(scan, task, inst_table, class_table)
    text = _vertex_text_numpy(xyz, _printed(rgb / 255))
    header = (_HEADER % (len(xyz), 0)).encode()
    w.call(_write_parts, path, (header, text))
    info.update(vertices=len(xyz), bytes=len(header) + text.size)
    return info


def _reference_form(task, rgb):
    """the dtype get_coords_color's rgb has in the reference, from the printed uint8 colours"""
    return rgb.astype(np.int64 if task in ('semantic_pred', 'offset_semantic_pred') else np.float64)


def _cloud(scan, task, backend, stage, inst_table, class_table):
    if task not in TASKS:
        raise ValueError(f'task {task!r}: one of {", ".join(TASKS)}')
    if backend != 'device' or task == 'input':            # (the input colours are one float32 expression)
        return _cloud_numpy(scan, task, inst_table, class_table)
    rgb, _ = _rgb_device(stage, scan, task, inst_table, class_table)
    keep = scan['semantic_label'] != _NONE
    return _xyz(scan, task)[keep], _reference_form(task, rgb.cpu().numpy())[keep]


def get_coords_color(prediction_path, room_name, task, backend='auto', instance_palette=None, class_palette=None):
    """``(xyz, rgb)`` of tools/visualization.py's ``get_coords_color`` for one room of a ``save_results`` tree,
    after its ``label != -100`` filter: xyz float32 [m, 3] (with the predicted offsets added for
    ``offset_semantic_pred``), rgb [m, 3] in 0..255 -- float32 for ``input``, float64 for ``semantic_gt`` and the
    instance tasks, int64 for the predicted classes.  A missing file raises and names the file
    (AssertionError for the prediction files, as the reference's asserts; FileNotFoundError for the four files
    every task opens); a class id outside the palette is an IndexError."""
    paint, read = _choose(backend, 'paint'), _choose(backend, 'read')
    inst_table = _palette(instance_palette, INSTANCE_PALETTE)
    class_table = _palette(class_palette, SCANNET_CLASS_PALETTE)
    stage = _Stage() if 'device' in (paint, read) else None
    scan = _file_scan(prediction_path, room_name, read, stage)
    return _cloud(scan, task, paint, stage, inst_table, class_table)


def colors_from_result(result, task, backend='auto', instance_palette=None, class_palette=None):
    """The same ``(xyz, rgb)`` straight from a ``forward_test`` result dict (``coords_float``, ``color_feats``,
    ``semantic_labels``, ``semantic_preds``, ``offset_preds``, ``pred_instances`` with run-length masks,
    ``gt_instances``; a ``LazyResults`` resolves on access): what ``get_coords_color`` returns for the tree
    ``save_results`` writes for this result, without the files.  The masks are painted from their runs, the
    confidences are taken at the four decimals the summary file keeps."""
    paint = _choose(backend, 'paint')
    inst_table = _palette(instance_palette, INSTANCE_PALETTE)
    class_table = _palette(class_palette, SCANNET_CLASS_PALETTE)
    stage = _Stage() if paint == 'device' else None
    return _cloud(_result_scan(result), task, paint, stage, inst_table, class_table)


def write_ply(verts, colors, indices, output_file, backend='auto'):
    """tools/visualization.py's ``write_ply``, byte for byte: the header (first line ``'ply '`` with its trailing
    space), ``'%f %f %f %d %d %d'`` per vertex with ``int(c * 255)`` colours (``colors=None``: zeros), ``'3 a b c'``
    per face.  float32 vertices with colours in 0..255 are printed by sg_viz_ply_vertices under
    ``backend='device'``; everything else by numpy.  Returns the description of the file (``formatted_by``,
    ``declined``, ``vertices``, ``bytes``)."""
    backend = _choose(backend, 'paint')
    verts = _host(verts)
    if verts.ndim != 2 or (len(verts) and verts.shape[1] < 3):
        raise ValueError('verts: an array [m, 3]')
    colors = np.zeros_like(verts) if colors is None else _host(colors)
    m = min(len(verts), len(colors))                       # (the reference zips the two)
    ints = _printed(colors[:m, :3]).reshape(m, 3)
    header = (_HEADER % (len(verts), 0 if indices is None else len(indices))).encode()
    faces = _face_text(indices)
    info = dict(path=output_file, formatted_by='numpy', declined=0, vertices=m)
    text = None
    if backend == 'device' and m and verts.dtype == np.float32:
        info['declined'] = int(((ints < 0) | (ints > 255)).sum())
        if not info['declined']:
            stage = _Stage()
            xyz = stage.upload(verts[:m, :3], np.float32)
            rgb = stage.upload(ints, np.uint8)
            pinned, _, total, _, declined = _vertex_text_device(stage, xyz, None, rgb, None, m)
            info['declined'] = declined
            if not declined:
                text = stage.to_host(pinned, total)[:total]
                info['formatted_by'] = 'device'
    if text is None:
        text = _vertex_text_numpy(verts[:m], ints)
    _write_parts(output_file, (header, text, faces))
    info['bytes'] = len(header) + len(text) + len(faces)
    return info


def save_visualizations(prediction_path, scan_ids, tasks, ply_dir, backend='auto', instance_palette=None,
                        class_palette=None):
    """``<ply_dir>/<scan>_<task>.ply`` for every scan and task of a ``save_results`` tree.  A scan's inputs are
    read once and shared by its tasks; the files are written on the writer threads (from pinned memory on the
    device path) and all are closed on return.  Returns one dict per file: ``path``, ``task``, ``vertices``,
    ``bytes``, ``formatted_by`` ('device' | 'numpy'), ``declined`` (what the kernels left to numpy) and, for
    ``instance_pred``, ``masks_reparsed`` (mask files the device parser left to numpy)."""
    paint, read = _choose(backend, 'paint'), _choose(backend, 'read')
    for task in tasks:
        if task not in TASKS:
            raise ValueError(f'task {task!r}: one of {", ".join(TASKS)}')
    inst_table = _palette(instance_palette, INSTANCE_PALETTE)
    class_table = _palette(class_palette, SCANNET_CLASS_PALETTE)
    os.makedirs(ply_dir, exist_ok=True)
    stage = _Stage() if 'device' in (paint, read) else None
    infos = []
    with _Writer() as w:
        for room in scan_ids:
            scan = _file_scan(prediction_path, room, read, stage)
            for task in tasks:
                path = osp.join(ply_dir, f'{room}_{task}.ply')
                infos.append(_cloud_file(w, stage if paint == 'device' else None, scan, task, path, inst_table,
                                         class_table))
    return infos
