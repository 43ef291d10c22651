"""The result files of a test run: what the reference's tools/test.py writes under ``--out`` (``save_npy``,
``save_pred_instances``, ``save_gt_instances``, ``save_panoptic``, tools/test.py:30-119, and the block of its
``main`` that calls them, :187-204), byte for byte, and readers for the text files.

    <out>/pred_instance/<scan>.txt                      "predicted_masks/<scan>_<i>.txt <label> <conf>" per instance
    <out>/pred_instance/predicted_masks/<scan>_<i>.txt  one '0' / '1' per point (the ScanNet benchmark's format)
    <out>/gt_instance/<scan>.txt                        one instance id per point
    <out>/panoptic/.../predictions/<frame>.label        uint32 words (the SemanticKITTI format)
    <out>/coords | colors | semantic_pred | ...         <scan>.npy

The reference decodes every run-length string to a dense vector and prints it with ``np.savetxt(fmt='%d')``:
0.2 s of one core per 150 000-point mask.  Here the strings are parsed to runs on the host (a few hundred numbers
per mask) and the text is produced from the runs:

  * ``backend='device'``: result_io.hip -- sg_mask_text_runs, sg_decimal_lines (with the NYU remap of
    ``save_gt_instance`` in front), sg_panoptic_kitti_words -- into a device buffer, one copy to pinned memory,
    and a thread pool writes the files from there.  Two pinned buffers alternate, so that formatting the next
    chunk overlaps writing the previous one.  Three inputs the entries do not take are formatted by the numpy
    path instead, with the same bytes: an ``nyu_id`` or ``learning_map_inv`` value outside int32, and panoptic
    words that are not uint32.
  * ``backend='numpy'``: the same bytes from vectorised numpy (no ``np.savetxt``), for tooling without a GPU.
  * ``backend='auto'``: numpy without a GPU; with one, what tools/save_results_bench.py measured to be faster on an
    MI355X host (``_AUTO`` below, figures in the README): the device for the mask and id text and for the
    readers, numpy for ``save_panoptic`` (half a megabyte per frame: a table lookup on the host costs less than
    the two copies).

Every file is closed when a function returns.  The readers (``read_mask``, ``read_int_lines``,
``load_pred_instances``) parse with sg_parse_mask_text / sg_parse_decimal_lines or with vectorised numpy and fall
back to ``split()`` for text neither of them accepts (hand-written files; numpy also leaves 19-digit values to it).
"""
import os
import os.path as osp
from concurrent.futures import ThreadPoolExecutor
from itertools import groupby

import numpy as np

from ..ops._args import choose_backend

__all__ = ['save_npy', 'save_pred_instances', 'save_gt_instances', 'save_panoptic', 'save_results', 'read_mask',
           'read_int_lines', 'load_pred_instances']

_THREADS = 8                   # file writers (a fixed number: the files are large, the disk is the limit)
_CHUNK_BYTES = 32 << 20        # text per device launch and pinned buffer
_NO_KEY = -2**31               # table entry of a class the panoptic class map lacks (result_io.hip: kIoNoKey)
_POW10 = np.array([10**k for k in range(1, 20)], dtype=np.uint64)
# what 'auto' means with a GPU present (module docstring): the text writers, save_panoptic, the readers
_AUTO = {'write': 'device', 'panoptic': 'numpy', 'read': 'device'}
# directory under --out -> key of the result dict, for the semantic task's arrays
_SEMANTIC_ARRAYS = (('coords', 'coords_float'), ('colors', 'color_feats'), ('semantic_pred', 'semantic_preds'),
                    ('semantic_label', 'semantic_labels'), ('offset_pred', 'offset_preds'),
                    ('offset_label', 'offset_labels'))


def _backend(backend, kind='write'):
    return choose_backend(backend, _AUTO[kind])


def _host(a):
    """numpy array of an array or tensor"""
    if hasattr(a, 'detach'):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def _write_file(path, data):
    with open(path, 'wb') as f:
        f.write(data)


class _Writer:
    """the file-writing threads of one save_* call; ``close`` waits for every file and re-raises a failure"""

    def __init__(self):
        self.pool = ThreadPoolExecutor(max_workers=_THREADS, thread_name_prefix='softgroup-save')
        self.futures = []

    def write(self, path, data):
        fut = self.pool.submit(_write_file, path, data)
        self.futures.append(fut)
        return fut

    def call(self, fn, *args):
        fut = self.pool.submit(fn, *args)
        self.futures.append(fut)
        return fut

    def close(self):
        self.pool.shutdown(wait=True)
        for f in self.futures:
            f.result()

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:
            self.pool.shutdown(wait=True)


class _Stage:
    """Device side of a save_* call: one device text buffer and two pinned buffers that alternate.  ``take``
    hands out the next pair once the files still being written from that pinned buffer are closed.  Small
    per-call constants (the NYU table, the class table, the read-back words, the scan workspace) are uploaded or
    allocated once per call, not per scan."""

    def __init__(self):
        import torch

        from .. import _lib as L
        self.torch, self.L, self.lib = torch, L, L.lib()
        self.dev = torch.device('cuda', torch.cuda.current_device())
        self.text = None
        self.pinned = [None, None]
        self.busy = [[], []]
        self.k = 0
        self.tables = {}
        self.meta = torch.empty(4, dtype=torch.int64, device=self.dev)
        self.ws = None

    def take(self, nbytes):
        torch = self.torch
        size = max(int(nbytes), _CHUNK_BYTES)
        if self.text is None or self.text.numel() < size:
            self.text = torch.empty(size, dtype=torch.uint8, device=self.dev)
        k = self.k
        self.k ^= 1
        for f in self.busy[k]:
            f.result()
        self.busy[k] = []
        if self.pinned[k] is None or self.pinned[k].numel() < size:
            self.pinned[k] = torch.empty(size, dtype=torch.uint8, pin_memory=True)
        return self.text, self.pinned[k], self.busy[k]

    def to_host(self, pinned, nbytes):
        """text[:nbytes] -> pinned[:nbytes], waited for; the numpy view of the pinned bytes"""
        if nbytes:
            pinned[:nbytes].copy_(self.text[:nbytes], non_blocking=True)
        self.torch.cuda.current_stream(self.dev).synchronize()
        return pinned.numpy()

    def upload(self, a, dtype):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.dev)

    def table(self, name, values):
        """int32 device copy of a small host table, uploaded on first use"""
        if name not in self.tables:
            self.tables[name] = self.upload(values, np.int32)
        return self.tables[name]

    def workspace(self, nbytes):
        if self.ws is None or self.ws.numel() < nbytes:
            self.ws = self.L.workspace(nbytes, self.dev)
        return self.ws


# ---- run-length strings -> runs ----------------------------------------------------------------------------
def _runs_of(rle):
    """(length, starts, ends): the 0-based runs rle_decode paints (softgroup/util/rle.py:30-38), ascending,
    disjoint and clipped to the mask, whatever order the string has them in"""
    length = int(rle['length'])
    tok = np.array(rle['counts'].split(), dtype=np.int64)
    starts = tok[0::2] - 1
    ends = np.minimum(starts + tok[1::2], length)
    if starts.size and starts.min() < 0:
        raise ValueError('run-length string with a start below 1')
    keep = ends > starts
    starts, ends = starts[keep], ends[keep]
    if starts.size > 1 and (starts[1:] <= ends[:-1]).any():          # unsorted, touching or overlapping: merge
        order = np.argsort(starts, kind='stable')
        starts, ends = starts[order], np.maximum.accumulate(ends[order])
        head = np.concatenate([[True], starts[1:] > ends[:-1]])
        starts, ends = starts[head], np.concatenate([ends[:-1][head[1:]], ends[-1:]])
    return length, starts, ends


def _mask_text_numpy(length, starts, ends):
    """np.savetxt(path, rle_decode(rle), fmt='%d')'s bytes as a uint8 array [length, 2]"""
    step = np.zeros(length + 1, dtype=np.uint8)         # +1 at a start, -1 (mod 256) at an end
    step[starts] = 1
    step[ends] = 255
    buf = np.empty((length, 2), dtype=np.uint8)
    np.cumsum(step[:-1], dtype=np.uint8, out=buf[:, 0])
    buf[:, 0] += 48
    buf[:, 1] = 10
    return buf


# ---- decimal lines ---------------------------------------------------------------------------------------------
def _as_int64(a, what):
    a = _host(a)
    if a.dtype.kind not in 'iub':
        raise TypeError(f'{what}: integer values expected, got {a.dtype}')
    if a.dtype == np.uint64 and a.size and a.max() > np.uint64(2**63 - 1):
        raise OverflowError(f'{what}: value outside int64')
    return np.ascontiguousarray(a.reshape(-1), dtype=np.int64)


def _remap_nyu(v, nyu_id):
    """ids = class * 1000 + instance with the 1-based class sent through nyu_id (what save_gt_instance does,
    tools/test.py:69-76); class 0 (ignore) stays 0 and does not read the table"""
    table = np.asarray(nyu_id)
    cls, inst = np.divmod(v, 1000)
    valid = cls != 0
    out = inst.copy()
    out[valid] += table[cls[valid] - 1] * 1000
    return out


def _int_lines_numpy(v):
    """np.savetxt(path, v, fmt='%d')'s bytes for int64 v, as a uint8 array"""
    n = v.size
    if n == 0:
        return np.empty(0, dtype=np.uint8)
    neg = v < 0
    mag = v.view(np.uint64).copy()
    mag[neg] = np.uint64(0) - mag[neg]                       # (two's complement: INT64_MIN -> 2^63)
    nd = np.searchsorted(_POW10, mag, side='right') + 1
    width = nd + neg + 1
    end = np.cumsum(width)
    out = np.empty(int(end[-1]), dtype=np.uint8)
    out[end - 1] = 10
    out[(end - width)[neg]] = 45
    for k in range(int(nd.max())):
        sel = nd > k
        out[end[sel] - 2 - k] = (mag[sel] // np.uint64(10**k) % np.uint64(10)).astype(np.uint8) + 48
    return out


def _digits(x):
    return len(str(abs(int(x))))


def _fits_int32(values):
    values = np.asarray(values, dtype=np.int64)
    return values.size > 0 and int(np.abs(values).max()) < 2**31 - 1


def _int_lines_device(stage, v, nyu_id):
    """(pinned numpy view, bytes, futures list) of the decimal lines of v, remap included"""
    L, lib = stage.L, stage.lib
    n = v.size
    big = max(abs(int(v.min())), abs(int(v.max()))) if n else 0
    table = None
    if nyu_id is not None:
        nyu = np.asarray(nyu_id, dtype=np.int64).reshape(-1)
        table = stage.table('nyu', nyu)
        big = max(big, (int(np.abs(nyu).max()) + 1) * 1000)
    cap = n * (_digits(big) + 2)
    text, pinned, busy = stage.take(cap)
    vals = stage.upload(v, np.int64)
    meta = stage.meta
    ws = stage.workspace(lib.sg_decimal_lines_workspace_bytes(n))
    L.check(lib.sg_decimal_lines(L.ptr(vals), n, L.ptr(table), 0 if table is None else table.numel(), L.ptr(text),
                                 cap, L.ptr(meta), L.ptr(ws), ws.numel(), L.stream()), 'sg_decimal_lines')
    total, bad, dropped = meta[:3].cpu().tolist()
    if bad:
        raise IndexError(f'{bad} instance ids whose semantic index is out of bounds for nyu_id of size {len(nyu_id)}')
    assert dropped == 0, 'sg_decimal_lines: text bound too small'
    return stage.to_host(pinned, total), total, busy


# ---- the writers -----------------------------------------------------------------------------------------------
def save_npy(root, name, scan_ids, arrs, backend='auto'):
    """``<root>/<name>/<scan>.npy`` for every scan (tools/test.py:30-37); ``np.save`` on the writer threads"""
    _backend(backend)
    root = osp.join(root, name)
    os.makedirs(root, exist_ok=True)
    with _Writer() as w:
        for i, arr in zip(scan_ids, arrs):
            w.call(np.save, osp.join(root, f'{i}.npy'), _host(arr))


def _mask_name(scan_id, k):
    """relative path of instance k's mask file: three digits, four from instance 1000 on"""
    return 'predicted_masks/%s_%s.txt' % (scan_id, format(k, '03d'))


def _summary(scan_id, insts, nyu_id):
    """the bytes of <scan>.txt: per instance the mask's relative path, the label (through the 1-based nyu_id
    table when there is one) and the confidence to four decimals.  An instance that names another scan is an
    AssertionError, as in the reference."""
    out = []
    for k, inst in enumerate(insts):
        assert inst['scan_id'] == scan_id, (inst['scan_id'], scan_id)
        label = inst['label_id'] if nyu_id is None else nyu_id[inst['label_id'] - 1]
        out.append('%s %s %s\n' % (_mask_name(scan_id, k), label, format(inst['conf'], '.4f')))
    return ''.join(out).encode()


def save_pred_instances(root, name, scan_ids, pred_insts, nyu_id=None, backend='auto'):
    """``<root>/<name>/<scan>.txt`` and ``<root>/<name>/predicted_masks/<scan>_<i>.txt`` (tools/test.py:40-65).
    ``pred_insts[s]``: the instance dicts of scan s, masks as ``{'length', 'counts'}`` run-length dicts."""
    backend = _backend(backend)
    root = osp.join(root, name)
    os.makedirs(root, exist_ok=True)
    stage = _Stage() if backend == 'device' else None
    with _Writer() as w:
        for scan_id, insts in zip(scan_ids, pred_insts):
            insts = list(insts)
            w.write(osp.join(root, f'{scan_id}.txt'), _summary(scan_id, insts, nyu_id))
            os.makedirs(osp.join(root, 'predicted_masks'), exist_ok=True)
            paths = [osp.join(root, _mask_name(scan_id, k)) for k in range(len(insts))]
            runs = [_runs_of(inst['pred_mask']) for inst in insts]
            if stage is None:
                for path, (length, starts, ends) in zip(paths, runs):
                    w.write(path, _mask_text_numpy(length, starts, ends))
                continue
            k = 0
            for length, group in groupby(runs, key=lambda r: r[0]):      # (one group: a scan's masks share N)
                group = list(group)
                _masks_device(stage, w, length, group, paths[k:k + len(group)])
                k += len(group)


def _masks_device(stage, w, length, runs, paths):
    """the mask files of `runs` (all over `length` points) through sg_mask_text_runs, a chunk of masks at a time"""
    L, lib = stage.L, stage.lib
    n_inst = len(runs)
    if length == 0:
        for p in paths:
            w.write(p, b'')
        return
    bounds = np.zeros(n_inst + 1, dtype=np.int64)
    np.cumsum([r[1].size for r in runs], out=bounds[1:])
    n_runs = int(bounds[-1])
    starts = stage.upload(np.concatenate([r[1] for r in runs]), np.int32)
    ends = stage.upload(np.concatenate([r[2] for r in runs]), np.int32)
    bounds_d = stage.upload(bounds, np.int64)
    row = 2 * length
    per = max(1, _CHUNK_BYTES // row)
    for first in range(0, n_inst, per):
        count = min(per, n_inst - first)
        text, pinned, busy = stage.take(count * row)
        L.check(lib.sg_mask_text_runs(L.ptr(starts), L.ptr(ends), L.ptr(bounds_d), n_runs, n_inst, length, first,
                                      count, L.ptr(text), text.numel(), L.stream()), 'sg_mask_text_runs')
        host = stage.to_host(pinned, count * row)
        for j in range(count):
            busy.append(w.write(paths[first + j], host[j * row:(j + 1) * row]))


def save_gt_instances(root, name, scan_ids, gt_insts, nyu_id=None, backend='auto'):
    """``<root>/<name>/<scan>.txt``: one instance id per line, through ``nyu_id`` when given
    (tools/test.py:68-88).  With an ``nyu_id`` entry outside int32, ``backend='device'`` formats with numpy."""
    backend = _backend(backend)
    root = osp.join(root, name)
    os.makedirs(root, exist_ok=True)
    on_device = backend == 'device' and (nyu_id is None or _fits_int32(nyu_id))
    stage = _Stage() if on_device else None
    with _Writer() as w:
        for i, gt in zip(scan_ids, gt_insts):
            path = osp.join(root, f'{i}.txt')
            v = _as_int64(gt, 'save_gt_instances')
            if stage is None:
                w.write(path, _int_lines_numpy(v if nyu_id is None else _remap_nyu(v, nyu_id)))
            else:
                host, total, busy = _int_lines_device(stage, v, nyu_id)
                busy.append(w.write(path, host[:total]))


def _kitti_table(learning_map_inv, num_classes):
    """The class map save_panoptic_single applies (tools/test.py:95-103) as an int64 table over the classes
    0 .. max key, _NO_KEY where the map has no key: train id k != 0 of learning_map_inv sits at class k + 10
    (k < 9: the things follow the stuff) or k - 9, and class num_classes means 0 unless a train id lands there.
    Keys a 16-bit class cannot take are left out."""
    by_class = {num_classes: 0}
    by_class.update({(k + 10 if k < 9 else k - 9): v for k, v in learning_map_inv.items() if k != 0})
    keys = [k for k in by_class if 0 <= k <= 0xFFFF]
    table = np.full(max(keys) + 1 if keys else 1, _NO_KEY, dtype=np.int64)
    for k in keys:
        table[int(k)] = int(by_class[k])
    return table


def _panoptic_numpy(arr, table):
    ids = arr >> 16
    cls = arr & 0xFFFF
    idx = cls.astype(np.int64)
    inside = (idx >= 0) & (idx < table.size)
    mapped = np.where(inside, table[np.where(inside, idx, 0)], _NO_KEY)
    miss = np.flatnonzero(mapped == _NO_KEY)
    if miss.size:
        raise KeyError(int(cls[miss[0]]))
    return (mapped.astype(arr.dtype) & 0xFFFF) | (ids << 16)


def _label_path(root, scan_id):
    """<root>/<scan>.label, the frame's 'velodyne' directory renamed to 'predictions' (wherever the word occurs in
    the scan id: the reference replaces in the whole string)"""
    return osp.join(root, (str(scan_id) + '.label').replace('velodyne', 'predictions'))


def save_panoptic(root, name, scan_ids, arrs, learning_map_inv, num_classes, backend='auto'):
    """``<root>/<name>/<scan>.label`` with 'velodyne' replaced by 'predictions' in the path: the panoptic
    words with the class sent through ``learning_map_inv`` (tools/test.py:91-119).  A class without an entry
    raises the reference's ``KeyError``.  Words that are not uint32, or a map value outside int32, make
    ``backend='device'`` format with numpy."""
    backend = _backend(backend, 'panoptic')
    root = osp.join(root, name)
    os.makedirs(root, exist_ok=True)
    paths = [_label_path(root, i) for i in scan_ids]
    for p in paths:
        os.makedirs(osp.dirname(p), exist_ok=True)
    table = _kitti_table(learning_map_inv, num_classes)
    on_device = backend == 'device' and _fits_int32(np.where(table == _NO_KEY, 0, table))
    stage = _Stage() if on_device else None
    with _Writer() as w:
        for path, arr in zip(paths, arrs):
            arr = _host(arr).reshape(-1)
            if arr.size == 0:
                raise ValueError('cannot call `vectorize` on size 0 inputs unless `otypes` is set')
            if stage is None or arr.dtype != np.uint32:
                w.write(path, np.ascontiguousarray(_panoptic_numpy(arr, table)))
                continue
            _panoptic_device(stage, w, path, arr, table)


def _panoptic_device(stage, w, path, arr, table):
    import ctypes as C
    L, lib = stage.L, stage.lib
    n = arr.size
    text, pinned, busy = stage.take(4 * n)
    lut = stage.table('kitti', table)
    words = stage.upload(arr.view(np.int32), np.int32)
    missing_host = (C.c_uint64 * 3)()
    rc = lib.sg_panoptic_kitti_words(L.ptr(words), n, L.ptr(lut), lut.numel(), L.ptr(text), L.ptr(stage.meta),
                                     C.addressof(missing_host), L.stream())
    if missing_host[0] and rc != 0:
        raise KeyError(int(missing_host[2]))
    L.check(rc, 'sg_panoptic_kitti_words')
    busy.append(w.write(path, stage.to_host(pinned, 4 * n)[:4 * n]))


def save_results(out_dir, results, eval_tasks, dataset, semantic_classes=None, backend='auto'):
    """Everything the reference's test script writes under ``--out`` (the end of its ``main``,
    tools/test.py:187-204) in one call.  ``results``: the result dicts of ``forward_test`` after
    ``collect_results`` (``LazyResults`` resolve on first access); ``eval_tasks``: the model's
    ``test_cfg.eval_tasks``; ``dataset``: anything with the dataset's ``NYU_ID`` and, for the panoptic task,
    ``learning_map_inv``; ``semantic_classes``: ``cfg.model.semantic_classes`` (default: the number of ``THING``
    and ``STUFF`` classes of the dataset)."""
    scan_ids = [res['scan_id'] for res in results]

    def column(key):
        return [res[key] for res in results]

    if 'semantic' in eval_tasks:
        for directory, key in _SEMANTIC_ARRAYS:
            save_npy(out_dir, directory, scan_ids, column(key), backend)
    if 'instance' in eval_tasks:
        nyu_id = getattr(dataset, 'NYU_ID', None)
        save_pred_instances(out_dir, 'pred_instance', scan_ids, column('pred_instances'), nyu_id, backend)
        save_gt_instances(out_dir, 'gt_instance', scan_ids, column('gt_instances'), nyu_id, backend)
    if 'panoptic' in eval_tasks:
        if semantic_classes is None:
            semantic_classes = len(dataset.THING) + len(dataset.STUFF)
        save_panoptic(out_dir, 'panoptic', scan_ids, column('panoptic_preds'), dataset.learning_map_inv,
                      semantic_classes, backend)


# ---- readers ------------------------------------------------------------------------------------------------------
def _read_bytes(path):
    with open(path, 'rb') as f:
        return f.read()


def _split_ints(data):
    return np.array(data.split(), dtype=np.int64)


def _parse_mask_numpy(data):
    buf = np.frombuffer(data, dtype=np.uint8)
    n = (buf.size + 1) // 2
    flags, seps = buf[0::2], buf[1::2]
    if ((flags & 0xFE) != 48).any() or (seps != 10).any():
        return None
    return flags[:n] == 49


def _parse_mask_device(data):
    import torch

    from .. import _lib as L
    lib = L.lib()
    dev = torch.device('cuda', torch.cuda.current_device())
    nbytes = len(data)
    n = (nbytes + 1) // 2
    if nbytes == 0 or nbytes >= 2**32:
        return None if nbytes else np.zeros(0, dtype=bool)
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    flags = torch.empty(n, dtype=torch.uint8, device=dev)
    meta = torch.empty(2, dtype=torch.int64, device=dev)
    L.check(lib.sg_parse_mask_text(L.ptr(text), nbytes, L.ptr(flags), None, L.ptr(meta), L.stream()),
            'sg_parse_mask_text')
    if meta.cpu()[1] != 0:
        return None
    return flags.cpu().numpy().view(bool)


def read_mask(path, backend='auto'):
    """A mask file -> bool array, one entry per line (any nonzero value is in: tools/eval_det.py:29-32)"""
    backend = _backend(backend, 'read')
    data = _read_bytes(path)
    mask = _parse_mask_device(data) if backend == 'device' else _parse_mask_numpy(data)
    if mask is None:
        mask = _split_ints(data) != 0
    return mask


def _parse_lines_numpy(data):
    """int64 values of "%d\\n" lines (optional '-', 1 to 18 digits; the last newline may be missing), or None for
    anything else: digit weights per byte, one segmented sum per line"""
    buf = np.frombuffer(data, dtype=np.uint8)
    if buf.size == 0:
        return np.zeros(0, dtype=np.int64)
    newline = np.flatnonzero(buf == 10)
    ends = newline if buf[-1] == 10 else np.append(newline, buf.size)
    starts = np.concatenate([[0], ends[:-1] + 1])
    neg = buf[starts] == 45
    n_digits = ends - starts - neg
    if (n_digits < 1).any() or (n_digits > 18).any():
        return None
    digit = (buf >= 48) & (buf <= 57)
    other = ~digit
    other[newline] = False
    other[starts[neg]] = False
    if other.any():
        return None
    line_end = np.repeat(ends, ends - starts + 1)[:buf.size]          # end of the line every byte belongs to
    power = np.clip(line_end - 1 - np.arange(buf.size), 0, 18)
    weighted = np.where(digit, (buf.astype(np.int64) - 48) * 10**power, 0)
    values = np.add.reduceat(weighted, starts)
    return np.where(neg, -values, values)


def _parse_lines_device(data):
    import torch

    from .. import _lib as L
    lib = L.lib()
    dev = torch.device('cuda', torch.cuda.current_device())
    nbytes = len(data)
    if nbytes == 0:
        return np.zeros(0, dtype=np.int64)
    if nbytes >= 2**31:
        return None
    cap = nbytes // 2 + 1
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    values = torch.empty(cap, dtype=torch.int64, device=dev)
    meta = torch.empty(2, dtype=torch.int64, device=dev)
    ws = L.workspace(lib.sg_parse_decimal_lines_workspace_bytes(nbytes), dev)
    L.check(lib.sg_parse_decimal_lines(L.ptr(text), nbytes, L.ptr(values), cap, L.ptr(meta), L.ptr(ws), ws.numel(),
                                       L.stream()), 'sg_parse_decimal_lines')
    lines, bad = meta.cpu().tolist()
    if bad:
        return None
    return values[:lines].cpu().numpy()


def read_int_lines(path, backend='auto'):
    """A file of decimal lines (``gt_instance/<scan>.txt``) -> int64 array"""
    backend = _backend(backend, 'read')
    data = _read_bytes(path)
    values = _parse_lines_device(data) if backend == 'device' else _parse_lines_numpy(data)
    if values is None:
        values = _split_ints(data)
    return values


def load_pred_instances(root, scan_id, backend='auto'):
    """The instances ``save_pred_instances`` wrote for a scan under ``root`` (= ``<out>/pred_instance``): dicts
    of ``scan_id``, ``label_id`` (as in the file: the NYU id where the writer had a table), ``conf`` and
    ``pred_mask`` (bool array)."""
    insts = []
    with open(osp.join(root, f'{scan_id}.txt')) as f:
        for line in f:
            fields = line.split()
            if not fields:
                continue
            mask_path, label, score = fields
            insts.append(dict(scan_id=scan_id, label_id=int(label), conf=float(score),
                              pred_mask=read_mask(osp.join(root, mask_path), backend)))
    return insts
