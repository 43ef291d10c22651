"""Inputs shared by test_cloud_io.py (CPU) and test_cloud_io_gpu.py: number spellings, grammar files, PLY bodies.
Every generator is seeded, so the two files see the same bytes."""
import math
import random
import struct
from fractions import Fraction

import numpy as np

MALFORMED_TOKENS = ['', '1_0', '0x10', '1d5', '1e', '1e+', '.', '+', '-', '+.', '1.2.3', '1e5.0', '--1', '1 2', 'abc',
                    'in', 'nano', '1,5', '\x101', '1' * 65, '0.' + '0' * 63]
DECLINED_TOKENS = ['inf', '-inf', '+Infinity', 'NaN', '-nan', 'INF', '1' * 20, '0.' + '1' * 20, '1e28', '1e-28',
                   '1234567890123456789e-28', '1e00005', '1e-10000', '0e10000', '123456789012345678.9e-27']


def _spell(rng, m, e):
    """one spelling of m * 10^e (m a digit string without sign), the decimal exponent of the digits staying e"""
    sign = rng.choice(['', '', '-', '+'])
    zeros = '0' * rng.choice([0, 0, 0, 1, 3])
    style = rng.randrange(5)
    if style == 0:                                   # digits, exponent written
        body, ex = zeros + m, e
    elif style == 1:                                 # a point inside
        k = rng.randrange(0, len(m) + 1)
        body, ex = zeros + m[:k] + '.' + m[k:], e + (len(m) - k)
        if body.startswith('.') and not m[k:]:
            body = '0' + body
    elif style == 2:                                 # '.ddd'
        body, ex = '.' + zeros + m, e + len(m) + len(zeros)
    elif style == 3:                                 # 'ddd.'
        body, ex = zeros + m + '.', e
    else:                                            # 0.ddd
        body, ex = '0.' + m, e + len(m)
    if body in ('.', ''):
        body = '0.'
    if ex == 0 and rng.random() < 0.5:
        return sign + body
    es = rng.choice(['e', 'E']) + rng.choice(['%d', '%+d', '%+03d', '%04d' if ex >= 0 else '%d']) % ex
    return sign + body + es


def random_tokens(n, seed=1):
    """tokens over the whole converted range: 1..19 digits, -27 <= e <= 27, every spelling mixed"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        nd = rng.randrange(1, 20)
        m = str(rng.randrange(10 ** (nd - 1), 10 ** nd)) if nd > 1 else str(rng.randrange(0, 10))
        if rng.random() < 0.1:
            m = m.rstrip('0') + '0' * rng.randrange(0, 4)
            m = (m or '0')[:19]
        e = rng.randrange(-27, 28)
        out.append(_spell(rng, m, e))
    return out


def midpoint_tokens(n, seed=2):
    """19-digit decimals within one unit of the midpoint of two adjacent doubles"""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        e = rng.randrange(-27, 9)
        # a double whose midpoint to the next one has 19 digits at exponent e
        x = rng.uniform(1.0, 9.999) * 10.0 ** (18 + e)
        y = math.nextafter(x, math.inf)
        mid = (Fraction(x) + Fraction(y)) / 2
        scaled = mid / Fraction(10) ** e
        base = scaled.numerator // scaled.denominator
        for m in (base - 1, base, base + 1):
            if 10 ** 18 <= m < 10 ** 19:
                out.append('%de%d' % (m, e))
    return out[:n]


def format_tokens(seed=3, count=20000):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-300.0, 300.0, size=count)
    out = {}
    for fmt in ('%.3f', '%.6f', '%.8f', '%.6e', '%.15g', '%.17g', '%.18e'):
        out[fmt] = [fmt % v for v in x]
    out['%d'] = ['%d' % v for v in x]
    out['repr32'] = [repr(float(np.float32(v))) for v in x]
    return out


def bits(x):
    return struct.pack('<d', x)


# ---- grammar files: (name, bytes, keyword arguments, malformed line or None) -----------------------------------
def grammar_files():
    f = []
    f.append(('spaces', b'1 2 3\n4 5 6\n', {}, None))
    f.append(('tabs', b'1\t2\t3\n4\t5\t6\n', {}, None))
    f.append(('mixed', b'  1 \t 2.5\t3e2  \n\t-4 +5 .6\t\n', {}, None))
    f.append(('comma', b'1,2,3\n4,5,6\n', dict(delimiter=','), None))
    f.append(('comma blanks', b' 1 , 2 ,3\n4,\t5 , 6 \n', dict(delimiter=','), None))
    f.append(('crlf', b'1 2 3\r\n4 5 6\r\n', {}, None))
    f.append(('crlf comma', b'1,2\r\n3,4\r\n', dict(delimiter=','), None))
    f.append(('no last newline', b'1 2 3\n4 5 6', {}, None))
    f.append(('blank lines', b'\n1 2\n\n   \n\t\r\n3 4\n\n', {}, None))
    f.append(('comments', b'# x y\n1 2\n  # more\n3 4\n#5 6', dict(comment='#'), None))
    f.append(('skip', b'x y z\nfoo\n1 2\n3 4\n', dict(skip_lines=2), None))
    f.append(('skip blank comment', b'h\n\n// c\n1;2\n/ c\n3;4\n', dict(skip_lines=1, comment='/', delimiter=';'), None))
    f.append(('skip all', b'1 2\n3 4\n', dict(skip_lines=5), None))
    f.append(('skip exactly', b'1 2\n3 4\n', dict(skip_lines=2), None))
    f.append(('empty', b'', {}, None))
    f.append(('only newline', b'\n', {}, None))
    f.append(('only header', b'x y z\n', dict(skip_lines=1), None))
    f.append(('one number', b'7', {}, None))
    f.append(('one number cols', b'7\n', dict(cols=1), None))
    f.append(('cols given', b'1 2 3\n4 5 6\n', dict(cols=3), None))
    f.append(('declined kinds', b'1 inf 3\n-nan 5 1e-300\n12345678901234567890 1 2\n', {}, None))
    f.append(('5 of 6', b'1 2 3 4 5 6\n1 2 3 4 5\n1 2 3 4 5 6\n', {}, 2))
    f.append(('7 of 6', b'1 2 3 4 5 6\n\n1 2 3 4 5 6 7\n1 2 3 4 5 6\n', {}, 3))
    f.append(('two bad', b'1 2\n1\n1 2\n1 2 3\n', {}, 2))
    f.append(('control byte', b'1.5 2.5\n1.\x105 2.5\n3 4\n', {}, 2))
    f.append(('high byte', b'1 2\n3 4\n5 \xe9\n', {}, 3))
    f.append(('bad token', b'1 2\n3 4x\n', {}, 2))
    f.append(('sign inside', b'1 2\n3 1-2\n5 6\n', {}, 2))
    f.append(('two points', b'1 2\n3 4\n5 1.2.3\n', {}, 3))
    f.append(('sign alone', b'1 +\n3 4\n', {}, 1))
    f.append(('point alone', b'1 2\n. 4\n', {}, 2))
    f.append(('sign and point', b'1,2\n3,-.\n', dict(delimiter=','), 2))
    f.append(('points at the ends', b'1. .2\n-3. +.4\n', {}, None))
    f.append(('underscore', b'1 2\n3 1_0\n', {}, 2))
    f.append(('empty field', b'1,2,3\n4,,6\n', dict(delimiter=','), 2))
    f.append(('trailing delimiter', b'1,2,3\n4,5,6,\n', dict(delimiter=',', cols=3), 2))
    f.append(('trailing delimiter 2', b'1,2,\n', dict(delimiter=',', cols=3), 1))
    f.append(('blank in field', b'1,2 3,4\n', dict(delimiter=',', cols=3), 1))
    f.append(('blank in field 2', b'1 2,,3\n', dict(delimiter=',', cols=3), 1))
    f.append(('only delimiter', b'1,2\n,\n', dict(delimiter=','), 2))
    f.append(('bad after skip', b'1 2 3\n1 2\n1 x\n', dict(skip_lines=1), 3))
    f.append(('comment mid line', b'1 2\n3 4 # no\n', dict(comment='#'), 2))
    f.append(('long token', b'1 2\n' + b'0' * 65 + b' 2\n', {}, 2))
    f.append(('64 byte token', b'1 2\n' + b'0' * 63 + b'7 2\n', {}, None))
    return f


def spelling_table(rows=4000, cols=6, seed=5):
    toks = random_tokens(rows * cols // 2, seed) + midpoint_tokens(rows * cols // 4, seed + 1)
    fm = format_tokens(seed + 2, rows * cols // 36 + 1)
    for v in fm.values():
        toks += v
    toks = toks[:rows * cols]
    random.Random(seed).shuffle(toks)
    lines = [' '.join(toks[r * cols:(r + 1) * cols]) for r in range(len(toks) // cols)]
    return ('\n'.join(lines) + '\n').encode()


def declined_table(rows=700, cols=6):
    """every 7th row holds one field the kernel declines; returns (bytes, indices of those rows)"""
    kinds = ['12345678901234567890', 'inf', '1e-300', '-NaN', '0.12345678901234567891']
    lines, which = [], []
    for r in range(rows):
        f = ['%.3f' % (r * 0.37 + c) for c in range(cols)]
        if r % 7 == 3:
            f[(r // 7) % cols] = kinds[(r // 7) % len(kinds)]
            which.append(r)
        lines.append(' '.join(f))
    return ('\n'.join(lines) + '\n').encode(), which


def offsets_table():
    """one column, rows of every length 1 .. 64 bytes (before the '\\n') in a fixed shuffled order, four times over:
    rows start at every offset modulo 16.  A row is blanks, zeros and up to 19 digits."""
    rng = random.Random(11)
    lengths = list(range(1, 65)) * 4
    rng.shuffle(lengths)
    lines = []
    for n in lengths:
        digits = str(rng.randrange(10 ** min(n, 19)))[:n]
        pad = n - len(digits)
        lead = rng.randrange(pad + 1) if rng.random() < 0.5 else 0
        lines.append(' ' * lead + '0' * (pad - lead) + digits)
    assert sorted(set(map(len, lines))) == list(range(1, 65))
    return ('\n'.join(lines) + '\n').encode()


# ---- PLY -----------------------------------------------------------------------------------------------------------
_STRUCT = {'float': 'f', 'float32': 'f', 'double': 'd', 'float64': 'd', 'uchar': 'B', 'uint8': 'B', 'char': 'b',
           'int8': 'b', 'ushort': 'H', 'uint16': 'H', 'short': 'h', 'int16': 'h', 'uint': 'I', 'uint32': 'I', 'int': 'i',
           'int32': 'i'}


def ply_bytes(fmt, props, rows, faces=(), extra_header=(), face_first=False):
    """a PLY file: fmt 'ascii' | 'binary_little_endian' | 'binary_big_endian', props [(type, name)], rows tuples"""
    vert = ['element vertex %d' % len(rows)] + ['property %s %s' % p for p in props]
    face = ['element face %d' % len(faces), 'property list uchar int vertex_indices']
    head = ['ply', 'format %s 1.0' % fmt, 'comment made by a test', 'obj_info nothing'] + list(extra_header)
    head += (face + vert) if face_first else (vert + face)
    head = ('\n'.join(head + ['end_header']) + '\n').encode()
    if fmt == 'ascii':
        body = ''.join(' '.join(repr(float(v)) if _STRUCT[t] in 'fd' else str(int(v)) for v, (t, _) in zip(r, props))
                       + '\n' for r in rows)
        body += ''.join('3 %d %d %d\n' % tuple(f) for f in faces)
        return head + body.encode()
    e = '<' if fmt == 'binary_little_endian' else '>'
    rec = struct.Struct(e + ''.join(_STRUCT[t] for t, _ in props))
    body = b''.join(rec.pack(*r) for r in rows)
    body += b''.join(struct.pack(e + 'Biii', 3, *f) for f in faces)
    return head + body


def scannet_rows(n=37, seed=4, label=False):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-5, 5, size=(n, 3)).astype(np.float32)
    rgba = rng.integers(0, 256, size=(n, 4))
    lab = rng.integers(0, 41, size=n)
    rows = [tuple(float(v) for v in xyz[i]) + tuple(int(v) for v in rgba[i]) + ((int(lab[i]),) if label else ())
            for i in range(n)]
    props = [('float', 'x'), ('float', 'y'), ('float', 'z'), ('uchar', 'red'), ('uchar', 'green'), ('uchar', 'blue'),
             ('uchar', 'alpha')] + ([('ushort', 'label')] if label else [])
    faces = [(0, 1, 2), (2, 3, 4), (1, 3, 5)]
    return props, rows, faces
