"""Delimited tables of decimal numbers (S3DIS rooms, STPLS3D tiles, ``.xyz`` / ``.txt`` / ``.csv`` exports, the
vertex lines of an ASCII PLY) -> float64 ``[rows, cols]``.

Rules, the same on both backends:

  * lines end with ``\\n`` (the last one may be missing); ``\\r`` is a blank like space and tab, so ``\\r\\n`` is fine;
  * a line of blanks alone is skipped; with ``comment`` a line whose first byte that is no blank equals it, too;
    ``skip_lines`` physical lines at the top are skipped whatever they hold; the rows are the other lines;
  * ``delimiter=None``: fields are separated by runs of blanks; ``delimiter=','`` (any printable byte): exactly one
    between two fields, blanks around a field are ignored, an empty field is malformed;
  * a number is ``[+-]? (D+ ('.' D*)? | '.' D+) ([eE] [+-]? D+)?`` or ``[+-]? (inf | infinity | nan)`` in any
    case, at most 64 bytes, and its value is what ``float()`` returns: correctly rounded;
  * a row with another field count than ``cols``, another token, or a byte outside printable ASCII, tab and ``\\r``
    is malformed: ``ValueError`` naming the lowest such physical line (1-based).

``parse_table_numpy`` is the definition: it splits by these rules, checks every token against the grammar and calls
``float()``.  ``parse_table(backend='device')`` runs cloud_io.hip: sg_text_table_count, one read-back, allocation,
sg_text_table_parse, one read-back.  The kernel converts digit strings of up to 19 digits whose decimal exponent lies
in -27..27 itself (decimal.h, exact integer arithmetic) and declines the rest -- longer strings, ``1e-300``, ``inf`` --
row by row; exactly those rows are parsed again by the definition and written into the result.  The two backends
return identical bytes.  Texts of 2^31 bytes and more are numpy's (``'device'`` raises).
"""
import re

import numpy as np

from ._args import _is_cuda, choose_backend

__all__ = ['parse_table', 'parse_table_numpy']

# what 'auto' means with a GPU present: the device call (bytes in memory to array) is ahead of np.loadtxt and
# pandas.read_csv on every file of tools/cloud_io_bench.py (profiles/cloud_io_bench.txt, figures in the README)
_AUTO = 'device'

_BLANKS = b' \t\r'
_NUMBER = rb'[+-]?(?:[0-9]+(?:\.[0-9]*)?|\.[0-9]+)(?:[eE][+-]?[0-9]+)?'
_TOKEN = re.compile(rb'(?:' + _NUMBER + rb'|[+-]?(?:inf|infinity|nan))\Z', re.I)
_PLAIN_RUN = re.compile(rb'(?:' + _NUMBER + rb' )*\Z')
_SPLIT = re.compile(rb'[ \t\r]+')
_MAX_TOKEN = 64
_LIMIT = 2**31


def _malformed(line):
    return ValueError(f'malformed table row at line {int(line)}')


def _byte_arg(value, what):
    """None or one printable, non-blank ASCII byte (str, bytes or int) -> int, -1 for None"""
    if value is None:
        return -1
    if isinstance(value, str):
        value = value.encode('latin-1', 'replace')
    if isinstance(value, (bytes, bytearray)):
        if len(value) != 1:
            raise ValueError(f'{what}: one byte')
        value = value[0]
    value = int(value)
    if not 0x20 < value < 0x7F:
        raise ValueError(f'{what}: a printable ASCII byte that is no blank')
    return value


def _delimiter_arg(delimiter):
    if isinstance(delimiter, (str, bytes)) and len(delimiter) and not delimiter.strip():
        return -1                                            # ' ', '\t': runs of blanks
    return _byte_arg(delimiter, 'delimiter')


def _row_tokens(line, delim):
    """the fields of one line (bytes without its '\\n'), or None when the line is no row of clean tokens"""
    if delim < 0:
        return _SPLIT.split(line.strip(_BLANKS))
    return [p.strip(_BLANKS) for p in line.split(bytes([delim]))]


def _row_values(line, delim, cols, number):
    """float64 values of one row, or ValueError for a malformed one"""
    if any(c > 0x7E or (c < 0x20 and c not in (9, 13)) for c in line):
        raise _malformed(number)
    tokens = _row_tokens(line, delim)
    if len(tokens) != cols:
        raise _malformed(number)
    out = []
    for t in tokens:
        if len(t) > _MAX_TOKEN or not _TOKEN.match(t):
            raise _malformed(number)
        out.append(float(t))
    return out


def _is_row(line, comment):
    s = line.strip(_BLANKS)
    return bool(s) and s[0] != comment


def _lines(buf):
    lines = buf.split(b'\n')
    if lines and lines[-1] == b'':
        lines.pop()
    return lines


def first_row_fields(buf, delimiter=None, skip_lines=0, comment=None):
    """field count of the first row of the text (None without one): what ``cols=None`` stands for"""
    delim, comment = _delimiter_arg(delimiter), _byte_arg(comment, 'comment')
    for k, line in enumerate(_lines(bytes(buf))):
        if k >= skip_lines and _is_row(line, comment):
            return len(_row_tokens(line, delim))
    return None


def _plain(buf, skip_lines, delim, cols):
    """The table by array operations and one float() per token, for text the checks below prove to be rows of exactly
    ``cols`` plain numbers: (values, lines, cols), or None (the line loop then decides)."""
    arr = np.frombuffer(buf, dtype=np.uint8)
    nl = arr == 10
    start_line = 0
    off = 0
    if skip_lines:
        pos = np.flatnonzero(nl)
        if len(pos) < skip_lines:
            return None
        off, start_line = int(pos[skip_lines - 1]) + 1, skip_lines
        arr, nl = arr[off:], nl[off:]
    if not arr.size:
        return None
    blank = (arr == 32) | (arr == 9) | (arr == 13)
    if ((arr > 0x7E) | ((arr < 0x20) & ~blank & ~nl)).any():
        return None
    cut = nl | (arr == delim) if delim >= 0 else nl            # a segment holds one field (one line without a delimiter)
    sep = blank | cut
    start = ~sep
    start[1:] &= sep[:-1]
    n_seg = int(cut.sum()) + 1
    seg_of = np.cumsum(cut) - cut                                # segment of every byte, its closing byte included
    tok_per_seg = np.bincount(seg_of[start], minlength=n_seg)
    line_of_seg = np.concatenate(([0], np.cumsum(nl[cut])))[:n_seg]
    n_lines = int(line_of_seg[-1]) + 1
    seg_per_line = np.bincount(line_of_seg, minlength=n_lines)
    tok_per_line = np.bincount(line_of_seg, weights=tok_per_seg, minlength=n_lines).astype(np.int64)
    empty = (tok_per_line == 0) & (seg_per_line == 1)
    rows = ~empty
    if not rows.any():
        return None
    if cols is None:
        cols = int(tok_per_line[np.argmax(rows)])
        if cols < 1:
            return None
    if delim >= 0:
        if (tok_per_seg[rows[line_of_seg]] != 1).any() or (seg_per_line[rows] != cols).any():
            return None
    elif (tok_per_line[rows] != cols).any():
        return None
    text = buf[off:]
    if delim >= 0:
        text = text.replace(bytes([delim]), b' ')
    tokens = text.split()
    if len(tokens) != int(rows.sum()) * cols or max(map(len, tokens)) > _MAX_TOKEN:
        return None
    digit, dot, sign = (arr >= 48) & (arr <= 57), arr == 46, (arr == 43) | (arr == 45)
    if (~sep & ~(digit | dot | sign)).any():
        if not _PLAIN_RUN.match(b' '.join(tokens) + b' '):     # exponents (or junk): the grammar, token by token
            return None
    else:
        # digits, points and signs alone: a number is a sign at its start at most, one point at most, one digit at least
        token_of = np.cumsum(start) - 1
        if (sign & ~start).any() or (np.bincount(token_of[digit], minlength=len(tokens)) < 1).any() or \
                (np.bincount(token_of[dot], minlength=len(tokens)) > 1).any():
            return None
    values = np.fromiter(map(float, tokens), dtype=np.float64, count=len(tokens)).reshape(-1, cols)
    lines = (np.flatnonzero(rows) + 1 + start_line).astype(np.int32)
    return values, lines, cols


def _as_bytes(data):
    if isinstance(data, (bytes, bytearray, memoryview)):
        return bytes(data)
    if _is_cuda(data):
        data = data.detach().cpu().numpy()
    data = np.ascontiguousarray(data)
    if data.dtype != np.uint8:
        raise ValueError('data: bytes or a uint8 array')
    return data.tobytes()


def parse_table_numpy(data, cols=None, delimiter=None, skip_lines=0, comment=None, dtype=np.float64,
                      return_lines=False):
    """The definition (module docstring): ``[rows, cols]`` of ``dtype`` from ``data`` (bytes or a uint8 array), with
    ``return_lines`` also the int32 1-based physical line of every row.  ``cols=None``: the field count of the first
    row.  A text without rows gives ``[0, cols or 0]``."""
    buf = _as_bytes(data)
    delim, com = _delimiter_arg(delimiter), _byte_arg(comment, 'comment')
    skip_lines = int(skip_lines)
    if skip_lines < 0 or (cols is not None and not 1 <= int(cols) <= 64):
        raise ValueError('skip_lines >= 0 and 1 <= cols <= 64')
    fast = None
    if com < 0 or bytes([com]) not in buf:
        fast = _plain(buf, skip_lines, delim, None if cols is None else int(cols))
    if fast is not None:
        values, lines, cols = fast
    else:
        rows, numbers = [], []
        for k, line in enumerate(_lines(buf)):
            if k < skip_lines or not _is_row(line, com):
                continue
            if cols is None:
                cols = len(_row_tokens(line, delim))
                if not 1 <= cols <= 64:
                    raise _malformed(k + 1)
            rows.append(_row_values(line, delim, int(cols), k + 1))
            numbers.append(k + 1)
        values = np.array(rows, dtype=np.float64).reshape(len(rows), int(cols or 0))
        lines = np.array(numbers, dtype=np.int32)
    values = values.astype(dtype, copy=False)
    return (values, lines) if return_lines else values


def _device_text(data):
    """(uint8 CUDA tensor, host bytes or None)"""
    import torch
    if _is_cuda(data):
        if data.dtype != torch.uint8 or data.dim() != 1:
            raise ValueError('data: a one-dimensional uint8 tensor')
        return data.contiguous(), None
    buf = _as_bytes(data)
    if not buf:
        return torch.empty(0, dtype=torch.uint8, device='cuda'), buf
    pinned = torch.empty(len(buf), dtype=torch.uint8, pin_memory=True)      # (one copy into memory the device reads)
    pinned.numpy()[:] = np.frombuffer(buf, dtype=np.uint8)
    text = pinned.cuda(non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return text, buf


def table_count_device(text, skip_lines=0, comment=-1):
    """sg_text_table_count on a uint8 CUDA tensor: (physical lines, rows, data offset); one read-back"""
    import torch

    from .. import _lib as L
    lib = L.lib()
    n = text.numel()
    meta = torch.empty(8, dtype=torch.int64, device=text.device)
    ws = L.workspace(lib.sg_text_table_workspace_bytes(n), text.device)
    L.check(lib.sg_text_table_count(L.ptr(text), n, skip_lines, comment, L.ptr(meta), L.ptr(ws), ws.numel(), L.stream()),
            'sg_text_table_count')
    return tuple(meta[:3].tolist())


def table_parse_device(text, cols, rows, delimiter=-1, skip_lines=0, comment=-1, values=None, row_status=None,
                       row_line=None):
    """sg_text_table_parse on a uint8 CUDA tensor into (given or new) device arrays: (values, row_status, row_line,
    meta as a list); one read-back"""
    import torch

    from .. import _lib as L
    lib = L.lib()
    n, dev = text.numel(), text.device
    values = torch.empty((rows, cols), dtype=torch.float64, device=dev) if values is None else values
    row_status = torch.empty(rows, dtype=torch.uint8, device=dev) if row_status is None else row_status
    row_line = torch.empty(rows, dtype=torch.int32, device=dev) if row_line is None else row_line
    meta = torch.empty(8, dtype=torch.int64, device=dev)
    ws = L.workspace(lib.sg_text_table_workspace_bytes(n), dev)
    L.check(lib.sg_text_table_parse(L.ptr(text), n, skip_lines, comment, delimiter, cols, rows, L.ptr(values),
                                    L.ptr(row_status), L.ptr(row_line), L.ptr(meta), L.ptr(ws), ws.numel(), L.stream()),
            'sg_text_table_parse')
    return values, row_status, row_line, meta.tolist()


def _line_bytes(buf, newlines, line):
    """physical line ``line`` (1-based) of buf, given the offsets of its newlines"""
    a = int(newlines[line - 2]) + 1 if line >= 2 else 0
    b = int(newlines[line - 1]) if line - 1 < len(newlines) else len(buf)
    return buf[a:b]


def _parse_table_device(data, cols, delim, skip_lines, com, return_lines, info):
    import torch
    text, buf = _device_text(data)
    n = text.numel()
    if n >= _LIMIT:
        raise ValueError("parse_table: backend='device' takes texts below 2**31 bytes")
    lines, rows, data_off = table_count_device(text, skip_lines, com)
    if cols is None and rows:
        # the first row's field count, on the host: from the text when it is there, else from the head of the data
        head, step = buf, 1 << 16
        cols = None
        while cols is None:
            if buf is None:
                head = text[data_off:data_off + step].cpu().numpy().tobytes()
                cut = head.rfind(b'\n')
                head = head if data_off + step >= n or cut < 0 else head[:cut + 1]
                cols = first_row_fields(head, None if delim < 0 else bytes([delim]), 0, None if com < 0 else com)
                if data_off + step >= n:
                    break
                step *= 16
            else:
                cols = first_row_fields(buf, None if delim < 0 else bytes([delim]), skip_lines, None if com < 0 else com)
                break
        if cols is None or not 1 <= cols <= 64:
            # (a first row of more than 64 fields: the line loop names it)
            return parse_table_numpy(_as_bytes(data), None, None if delim < 0 else bytes([delim]), skip_lines,
                                     None if com < 0 else com, np.float64, True)
    if not rows:
        empty = torch.empty((0, int(cols or 0)), dtype=torch.float64, device=text.device)
        return empty, torch.empty(0, dtype=torch.int32, device=text.device)
    values, status, row_line, meta = table_parse_device(text, int(cols), rows, delim, skip_lines, com)
    if meta[6] or meta[1] != rows:
        raise RuntimeError(f'parse_table: the text changed between the two passes ({rows} rows, then {meta[1]})')
    if meta[4]:
        raise _malformed(meta[5])
    info['declined'] = int(meta[3])
    if meta[3]:
        idx = torch.nonzero(status & 1).flatten()
        where = row_line[idx].cpu().numpy()
        buf = _as_bytes(data) if buf is None else buf
        newlines = np.flatnonzero(np.frombuffer(buf, dtype=np.uint8) == 10)
        patch = np.array([_row_values(_line_bytes(buf, newlines, int(k)), delim, int(cols), int(k)) for k in where],
                         dtype=np.float64).reshape(len(where), int(cols))
        values[idx] = torch.from_numpy(patch).to(values.device)
    return values, row_line


def parse_table(data, cols=None, delimiter=None, skip_lines=0, comment=None, dtype=np.float64, backend='auto',
                return_lines=False, info=None):
    """``data`` (bytes, a uint8 numpy array or a uint8 CUDA tensor) -> ``[rows, cols]`` of ``dtype`` (float64, or
    float32: one rounding from the double); a CUDA tensor in gives a CUDA tensor out, anything else a numpy array.
    Rules and errors in the module docstring; ``cols=None`` takes the first row's field count.  ``backend``:
    ``'device'`` (cloud_io.hip), ``'numpy'`` (the definition), ``'auto'`` (``_AUTO`` with a GPU; numpy from 2^31 bytes).
    ``return_lines``: also the int32 physical line of every row.  ``info`` (a dict) receives ``backend`` and
    ``declined``, the rows the kernel left to the definition."""
    import torch
    np_dtype = np.dtype(dtype if not isinstance(dtype, torch.dtype) else {torch.float32: np.float32,
                                                                         torch.float64: np.float64}[dtype])
    if np_dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError('dtype: float32 or float64')
    info = {} if info is None else info
    delim, com = _delimiter_arg(delimiter), _byte_arg(comment, 'comment')
    skip_lines = int(skip_lines)
    if skip_lines < 0 or (cols is not None and not 1 <= int(cols) <= 64):
        raise ValueError('skip_lines >= 0 and 1 <= cols <= 64')
    cuda_in = _is_cuda(data)
    nbytes = data.numel() if torch.is_tensor(data) else len(data)
    chosen = choose_backend(backend, _AUTO)
    if backend == 'auto' and nbytes >= _LIMIT:
        chosen = 'numpy'
    info.update(backend=chosen, declined=0)
    if chosen == 'device':
        values, lines = _parse_table_device(data, None if cols is None else int(cols), delim, skip_lines, com,
                                            return_lines, info)
        if torch.is_tensor(values):
            values = values.to(torch.float32) if np_dtype == np.float32 else values
            if not cuda_in:
                values, lines = values.cpu().numpy(), lines.cpu().numpy()
        else:
            values = values.astype(np_dtype, copy=False)
    else:
        values, lines = parse_table_numpy(data, cols, delimiter, skip_lines, comment, np_dtype, True)
    if cuda_in and not torch.is_tensor(values):
        values, lines = torch.from_numpy(values).cuda(), torch.from_numpy(lines).cuda()
    return (values, lines) if return_lines else values
