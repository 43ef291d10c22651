"""Raw point-cloud files -> arrays, in the form ``TestTransform``, ``tile_cloud`` and ``voxel_downsample`` take.

    read_table   a delimited text table (S3DIS ``x y z r g b`` rooms, STPLS3D ``.csv`` tiles, ``.xyz`` / ``.txt``
                 exports): what the reference's preparations read with ``pandas.read_csv``
                 (dataset/s3dis/prepare_data_inst.py:65,84, dataset/stpls3d/prepare_data_inst_instance_stpls3d.py:39,77)
    read_ply     the ``vertex`` element of a PLY file, ASCII or binary of either byte order: what
                 dataset/scannetv2/prepare_data_inst.py:38,53,58 reads through ``plyfile`` (not needed here)
    read_cloud   either of them, or a KITTI ``.bin`` (softgroup/data/kitti.py:63), as ``xyz`` / ``rgb`` / labels

Text is parsed by ``ops.text.parse_table`` (rules, limits and the two backends are described there); with
``backend='device'`` the file is read into pinned memory, copied to the device and parsed by cloud_io.hip.  Binary PLY
bodies and ``.bin`` files are a ``np.frombuffer`` on the host: the work is a copy.
"""
import os.path as osp

import numpy as np

from ..ops import text as T
from ..ops._args import choose_backend

__all__ = ['read_table', 'read_ply', 'read_cloud']

_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2',
              'uint16': 'u2', 'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4',
              'double': 'f8', 'float64': 'f8'}
_PLY_FORMATS = {'ascii': None, 'binary_little_endian': '<', 'binary_big_endian': '>'}
_PLY_KEYS = {'red': 'r', 'green': 'g', 'blue': 'b', 'label': 'semantic'}


def _choose(backend):
    return choose_backend(backend, T._AUTO)


def _read_bytes(path):
    with open(path, 'rb') as f:
        return f.read()


def _read_device(path):
    """the file's bytes as a uint8 CUDA tensor, through a pinned buffer"""
    import torch
    n = osp.getsize(path)
    if n == 0:
        return torch.empty(0, dtype=torch.uint8, device='cuda')
    pinned = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    with open(path, 'rb') as f:
        got = f.readinto(memoryview(pinned.numpy()))
    if got != n:
        raise OSError(f'{path}: read {got} of {n} bytes')
    text = pinned.cuda(non_blocking=True)
    torch.cuda.current_stream().synchronize()                # (the pinned buffer is released on return)
    return text


def read_table(path, cols=None, delimiter=None, skip_lines=0, comment=None, dtype=np.float64, backend='auto', info=None):
    """The table in a text file -> ``[rows, cols]`` (``ops.text.parse_table``): a numpy array under the numpy backend,
    a CUDA tensor under ``backend='device'`` (the file goes through pinned memory to the device and is parsed there).
    A file of 2^31 bytes and more is numpy's under ``'auto'``."""
    backend = _choose(backend)
    if backend == 'device' and osp.getsize(path) < T._LIMIT:
        data = _read_device(path)
    elif backend == 'device':
        raise ValueError(f"{path}: backend='device' takes files below 2**31 bytes")
    else:
        data = _read_bytes(path)
    return T.parse_table(data, cols, delimiter, skip_lines, comment, dtype, backend, info=info)


def _ply_header(buf, path):
    """(format, vertex count, [(name, numpy type code)], offset of the body)"""
    end = buf.find(b'end_header')
    stop = buf.find(b'\n', end) if end >= 0 else -1
    if not buf.startswith(b'ply') or stop < 0:
        raise ValueError(f'{path}: not a PLY file (no "ply" ... "end_header" header)')
    fmt, elements = None, []
    for raw in buf[:stop].split(b'\n')[1:]:
        words = raw.decode('latin-1').split()
        if not words or words[0] in ('comment', 'obj_info', 'end_header'):
            continue
        if words[0] == 'format':
            if len(words) != 3 or words[1] not in _PLY_FORMATS or words[2] != '1.0':
                raise ValueError(f'{path}: PLY format {" ".join(words[1:])!r}: ascii, binary_little_endian or '
                                 'binary_big_endian 1.0')
            fmt = words[1]
        elif words[0] == 'element' and len(words) == 3:
            elements.append((words[1], int(words[2]), []))
        elif words[0] == 'property' and elements:
            elements[-1][2].append(words[1:])
        else:
            raise ValueError(f'{path}: PLY header line {raw!r}')
    if fmt is None:
        raise ValueError(f'{path}: PLY header without a format line')
    if not elements or elements[0][0] != 'vertex':
        raise ValueError(f'{path}: the vertex element is not the first element of the PLY file '
                         f'({[e[0] for e in elements]})')
    props = []
    for p in elements[0][2]:
        if p[0] == 'list':
            raise ValueError(f'{path}: a list property ({p[-1]}) inside the vertex element')
        if len(p) != 2 or p[0] not in _PLY_TYPES:
            raise ValueError(f'{path}: PLY property {" ".join(p)!r}')
        props.append((p[1], _PLY_TYPES[p[0]]))
    if not props or elements[0][1] < 0:
        raise ValueError(f'{path}: a vertex element without properties')
    return fmt, elements[0][1], props, stop + 1


def read_ply(path, backend='auto'):
    """``{property name: array}`` of the ``vertex`` element of a PLY file, every property in its declared type (numpy
    arrays).  ``format ascii 1.0``: the vertex lines go through ``parse_table`` (``backend`` as there) and are cast;
    ``binary_little_endian`` / ``binary_big_endian``: a structured ``np.frombuffer``.  ``comment`` and ``obj_info``
    lines and the elements behind ``vertex`` (faces) are ignored.  ``ValueError`` for a ``list`` property inside
    ``vertex``, for a file whose first element is not ``vertex``, and for a body that ends early."""
    buf = _read_bytes(path)
    fmt, count, props, body = _ply_header(buf, path)
    if _PLY_FORMATS[fmt] is not None:
        dt = np.dtype([(name, _PLY_FORMATS[fmt] + code) for name, code in props])
        if len(buf) - body < count * dt.itemsize:
            raise ValueError(f'{path}: truncated PLY body ({len(buf) - body} bytes for {count} vertices of '
                             f'{dt.itemsize})')
        rec = np.frombuffer(buf, dtype=dt, count=count, offset=body)
        return {name: np.ascontiguousarray(rec[name]).astype(code) for name, code in props}
    arr = np.frombuffer(buf, dtype=np.uint8, offset=body) if len(buf) > body else np.empty(0, np.uint8)
    newlines = np.flatnonzero(arr == 10)
    if count == 0:
        stop = 0
    elif len(newlines) >= count:
        stop = int(newlines[count - 1]) + 1
    elif len(newlines) == count - 1 and arr.size and arr[-1] != 10:
        stop = arr.size
    else:
        raise ValueError(f'{path}: truncated PLY body ({len(newlines)} lines for {count} vertices)')
    values = T.parse_table(arr[:stop], len(props), None, 0, None, np.float64, _choose(backend))
    if len(values) != count:
        raise ValueError(f'{path}: truncated PLY body ({len(values)} vertex lines for {count} vertices)')
    return {name: values[:, k].astype(code) for k, (name, code) in enumerate(props)}


def _format_of(path, fmt):
    if fmt != 'auto':
        if fmt not in ('ply', 'bin', 'csv', 'table'):
            raise ValueError(f"format {fmt!r}: one of 'auto', 'ply', 'bin', 'csv', 'table'")
        return fmt
    return {'.ply': 'ply', '.bin': 'bin', '.csv': 'csv'}.get(osp.splitext(path)[1].lower(), 'table')


def _assemble(columns, take, rgb, xp):
    """the result dict from named columns; ``take(k)`` is column k as float64, ``xp`` numpy or torch"""
    names = [None if c in (None, '_') else str(c) for c in columns]
    used = [c for c in names if c is not None]
    if len(set(used)) != len(used):
        raise ValueError(f'columns {columns!r}: a name appears twice')
    if rgb not in ('unit', 'raw'):
        raise ValueError(f"rgb {rgb!r}: 'unit' or 'raw'")
    at = {c: k for k, c in enumerate(names) if c is not None}
    if not all(c in at for c in 'xyz'):
        raise ValueError(f"columns {columns!r}: 'x', 'y' and 'z' are needed")
    out = {'xyz': xp.stack([take(at[c]) for c in 'xyz'], 1).astype('float32') if xp is np else
           xp.stack([take(at[c]) for c in 'xyz'], 1).to(xp.float32)}
    rest = [c for c in used if c not in 'xyz']
    if all(c in at for c in 'rgb'):
        c3 = xp.stack([take(at[c]) for c in 'rgb'], 1)
        if rgb == 'unit':
            c3 = c3 / 127.5 - 1
        out['rgb'] = c3.astype('float32') if xp is np else c3.to(xp.float32)
        rest = [c for c in rest if c not in 'rgb']
    for c in rest:
        v = take(at[c])
        if c in ('semantic', 'instance'):
            ok = xp.isfinite(v) & (v == xp.trunc(v))
            if not bool(ok.all()):
                raise ValueError(f'column {c!r}: a label that is not finite or not integral')
            out[c + '_labels'] = v.astype('int64') if xp is np else v.to(xp.int64)
        else:
            out[c] = v
    return out


def read_cloud(path, format='auto', columns=('x', 'y', 'z', 'r', 'g', 'b'), rgb='unit', delimiter=None, skip_lines=0,
               comment=None, backend='auto', info=None):
    """A point cloud file -> dict of ``xyz`` float32 [N, 3]; ``rgb`` float32 [N, 3] when r, g and b are there
    (``rgb='unit'``: ``float32(float64(c) / 127.5 - 1)``, the scaling of the reference's preparations; ``'raw'``:
    ``float32(c)``); ``semantic_labels`` / ``instance_labels`` int64 for columns named ``semantic`` / ``instance``
    (``ValueError`` for a value that is not finite or not integral); every other named column as float64 under its
    name.  ``columns`` names the columns of a text table in order, ``None`` or ``'_'`` drops one.

    ``format='auto'`` goes by the suffix: ``.ply`` -> ``read_ply`` with x, y, z, red, green, blue and label mapped to
    the same keys (``columns`` is ignored); ``.bin`` -> KITTI float32 [N, 4]: ``xyz`` and ``intensity``; ``.csv`` ->
    a table with delimiter ``,`` unless one is given; anything else -> a table separated by blanks.  Arrays are numpy
    under the numpy backend and CUDA tensors under ``backend='device'``; ``info`` (a dict) receives ``format``,
    ``backend`` and ``declined``."""
    info = {} if info is None else info
    fmt = _format_of(path, format)
    backend = _choose(backend)
    info.update(format=fmt, backend=backend, declined=0)
    if fmt == 'bin':
        pts = np.fromfile(path, dtype=np.float32)
        if pts.size % 4:
            raise ValueError(f'{path}: {pts.size} float32 values are no [N, 4] array')
        pts = pts.reshape(-1, 4)
        out = {'xyz': np.ascontiguousarray(pts[:, :3]), 'intensity': np.ascontiguousarray(pts[:, 3])}
    elif fmt == 'ply':
        props = read_ply(path, backend)
        names = list(props)
        out = _assemble([_PLY_KEYS.get(n, n) for n in names], lambda k: props[names[k]].astype(np.float64), rgb, np)
    else:
        if fmt == 'csv' and delimiter is None:
            delimiter = ','
        values = read_table(path, len(columns), delimiter, skip_lines, comment, np.float64, backend, info)
        if backend == 'device':
            import torch
            return _assemble(columns, lambda k: values[:, k], rgb, torch)
        return _assemble(columns, lambda k: values[:, k], rgb, np)
    if backend == 'device':
        import torch
        out = {k: torch.from_numpy(v).cuda() for k, v in out.items()}
    return out
