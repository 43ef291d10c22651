"""Raw point-cloud files on the CPU: decimal.h's routine against float() bit for bit (sg_decimal_to_double_host),
parse_table_numpy (the definition) on the grammar, read_ply, read_cloud and tools/read_cloud.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_io_cases as cc  # noqa: E402

from softgroup_amd import _lib  # noqa: E402
from softgroup_amd.ops import text as T  # noqa: E402
from softgroup_amd.util import read_cloud, read_ply, read_table, write_ply  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 12345.678


def convert(tokens):
    """(values float64, status uint8) of sg_decimal_to_double_host; the value slots start as SENTINEL"""
    enc = [t.encode('latin-1') for t in tokens]
    ln = np.array([len(e) for e in enc], dtype=np.int32)
    begin = (np.cumsum(ln, dtype=np.int64) - ln).astype(np.int64)
    text = np.frombuffer(b''.join(enc) + b'\0', dtype=np.uint8)
    val = np.full(len(enc), SENTINEL, dtype=np.float64)
    st = np.full(len(enc), 255, dtype=np.uint8)
    rc = _lib.lib().sg_decimal_to_double_host(text.ctypes.data, begin.ctypes.data, ln.ctypes.data, len(enc),
                                              val.ctypes.data, st.ctypes.data)
    assert rc == 0
    return val, st


def assert_exact(tokens):
    val, st = convert(tokens)
    ref = np.array([float(t) for t in tokens], dtype=np.float64)
    assert int((st != 0).sum()) == 0, [tokens[i] for i in np.flatnonzero(st != 0)[:5]]
    wrong = np.flatnonzero(val.view(np.uint64) != ref.view(np.uint64))
    assert wrong.size == 0, [(tokens[i], val[i].hex(), ref[i].hex()) for i in wrong[:5]]


def test_decimal_random_tokens_over_the_whole_range():
    tokens = cc.random_tokens(200000)
    assert any(t.startswith('.') or t[1:2] == '.' and t[0] in '+-' for t in tokens)
    assert any('E+' in t for t in tokens) and any(t.startswith('000') for t in tokens)
    assert_exact(tokens)


def test_decimal_near_midpoints():
    tokens = cc.midpoint_tokens(50000)
    assert len(tokens) == 50000 and all(len(t.split('e')[0]) == 19 for t in tokens)
    assert_exact(tokens)


def test_decimal_exact_ties_resolve_to_even():
    val, st = convert(['9007199254740993', '9007199254740995', '9007199254740992.5'])
    assert st.tolist() == [0, 0, 0]
    assert val.tolist() == [9007199254740992.0, 9007199254740996.0, 9007199254740992.0]
    assert_exact(['9007199254740993', '9007199254740995', '9007199254740992.5', '-9007199254740993'])


def test_decimal_zeros_keep_their_sign():
    val, st = convert(['-0.0', '0e9999', '-.0e-5', '+0', '-0e-9999', '0.' + '0' * 40])
    assert st.tolist() == [0] * 6
    assert [cc.bits(v) for v in val] == [cc.bits(x) for x in (-0.0, 0.0, -0.0, 0.0, -0.0, 0.0)]


@pytest.mark.parametrize('fmt', ['%.3f', '%.6f', '%.8f', '%d', '%.6e', '%.15g', '%.17g', 'repr32', '%.18e'])
def test_decimal_printed_formats_are_never_declined(fmt):
    tokens = cc.format_tokens()[fmt]
    assert len(tokens) == 20000
    assert_exact(tokens)


def test_decimal_outside_the_range_is_declined_and_junk_is_malformed():
    val, st = convert(cc.DECLINED_TOKENS)
    assert st.tolist() == [1] * len(cc.DECLINED_TOKENS), list(zip(cc.DECLINED_TOKENS, st))
    assert (val == SENTINEL).all()
    val, st = convert(cc.MALFORMED_TOKENS)
    assert st.tolist() == [2] * len(cc.MALFORMED_TOKENS), list(zip(cc.MALFORMED_TOKENS, st))
    assert (val == SENTINEL).all()
    # the edges: 19 digits, e = +-27 and 4 exponent digits are converted
    assert_exact(['1234567890123456789', '1e27', '1e-27', '9999999999999999999e27', '1e-0027', '0.0000000000000000001e-8'])
    # and the definition agrees on what a token is
    for t in cc.MALFORMED_TOKENS:
        assert not T._TOKEN.match(t.encode('latin-1')) or len(t) > 64, t
    for t in cc.DECLINED_TOKENS:
        assert T._TOKEN.match(t.encode('latin-1')), t


# ---- parse_table_numpy ----------------------------------------------------------------------------------------------
def reference_rows(data, cols=None, delimiter=None, skip_lines=0, comment=None):
    """the rules spelled out once more, line by line, without any fast path"""
    rows, lines = [], []
    phys = data.split(b'\n')
    if phys[-1] == b'':
        phys.pop()
    for k, line in enumerate(phys):
        s = line.strip(b' \t\r')
        if k < skip_lines or not s or (comment is not None and s[:1] == comment.encode()):
            continue
        toks = s.split() if delimiter is None else [p.strip(b' \t\r') for p in line.split(delimiter.encode())]
        rows.append([float(t) for t in toks])
        lines.append(k + 1)
    width = cols if cols is not None else (len(rows[0]) if rows else 0)
    return np.array(rows, dtype=np.float64).reshape(len(rows), width), np.array(lines, dtype=np.int32)


@pytest.mark.parametrize('case', cc.grammar_files(), ids=lambda c: c[0])
def test_parse_table_numpy_on_the_grammar(case):
    name, data, kw, bad_line = case
    if bad_line is not None:
        with pytest.raises(ValueError, match=rf'line {bad_line}\b'):
            T.parse_table_numpy(data, **kw)
        return
    got, lines = T.parse_table_numpy(data, return_lines=True, **kw)
    ref, ref_lines = reference_rows(data, **kw)
    assert got.dtype == np.float64 and got.shape == ref.shape
    assert got.tobytes() == ref.tobytes()
    assert lines.dtype == np.int32 and np.array_equal(lines, ref_lines)
    as32 = T.parse_table_numpy(data, dtype=np.float32, **kw)
    assert as32.dtype == np.float32 and as32.tobytes() == ref.astype(np.float32).tobytes()
    # the same text as a uint8 array, and through parse_table's numpy backend
    again = T.parse_table(np.frombuffer(data, dtype=np.uint8), backend='numpy', **kw)
    assert again.tobytes() == ref.tobytes()


def test_parse_table_numpy_fast_path_equals_the_line_loop():
    for data, kw in ((cc.spelling_table(rows=300), {}), (cc.declined_table()[0], {}), (cc.offsets_table(), dict(cols=1)),
                     (cc.spelling_table(rows=200).replace(b' ', b' , '), dict(delimiter=','))):
        assert T._plain(data, 0, T._delimiter_arg(kw.get('delimiter')), kw.get('cols')) is not None or b'inf' in data
        got, lines = T.parse_table_numpy(data, return_lines=True, **kw)
        ref, ref_lines = reference_rows(data, **kw)
        assert got.tobytes() == ref.tobytes() and np.array_equal(lines, ref_lines)


def test_parse_table_arguments():
    with pytest.raises(ValueError):
        T.parse_table(b'1 2\n', delimiter=',,')
    with pytest.raises(ValueError):
        T.parse_table(b'1 2\n', cols=65)
    with pytest.raises(ValueError):
        T.parse_table(b'1 2\n', backend='cuda')
    with pytest.raises(ValueError):
        T.parse_table(b'1 2\n', dtype=np.int32)
    assert T._AUTO in ('numpy', 'device')
    assert T.parse_table(b'1 2\n', delimiter=' ').tolist() == [[1.0, 2.0]]


# ---- read_ply -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt', ['ascii', 'binary_little_endian', 'binary_big_endian'])
@pytest.mark.parametrize('label', [False, True])
def test_read_ply_scannet_layouts(tmp_path, fmt, label):
    props, rows, faces = cc.scannet_rows(label=label)
    path = tmp_path / 'scene.ply'
    path.write_bytes(cc.ply_bytes(fmt, props, rows, faces))
    got = read_ply(str(path), backend='numpy')
    assert list(got) == [n for _, n in props]
    want = {'float': np.float32, 'uchar': np.uint8, 'ushort': np.uint16}
    for k, (t, n) in enumerate(props):
        assert got[n].dtype == want[t] and got[n].shape == (len(rows),)
        assert got[n].tobytes() == np.array([r[k] for r in rows], dtype=want[t]).tobytes(), n


def test_read_ply_type_spellings_and_doubles(tmp_path):
    props = [('float32', 'x'), ('float64', 'y'), ('double', 'z'), ('uint8', 'red'), ('int16', 'a'), ('int', 'b'),
             ('uint', 'c'), ('char', 'd')]
    rows = [(0.1, 0.1, -2.5e-7, 255, -300, -70000, 4000000000, -7), (1.5, 1 / 3, 7.0, 0, 12, 5, 6, 8)]
    for fmt in ('ascii', 'binary_little_endian', 'binary_big_endian'):
        path = tmp_path / f'{fmt}.ply'
        path.write_bytes(cc.ply_bytes(fmt, props, rows))
        got = read_ply(str(path), backend='numpy')
        assert [got[n].dtype.str[1:] for _, n in props] == ['f4', 'f8', 'f8', 'u1', 'i2', 'i4', 'u4', 'i1']
        assert got['y'].tolist() == [0.1, 1 / 3] and got['x'].tolist() == [float(np.float32(0.1)), 1.5]
        assert got['c'].tolist() == [4000000000, 6] and got['b'].tolist() == [-70000, 5] and got['d'].tolist() == [-7, 8]


def test_read_ply_reads_what_write_ply_wrote(tmp_path):
    rng = np.random.default_rng(0)
    verts = rng.uniform(-3, 3, size=(50, 3)).astype(np.float32)
    colors = rng.integers(0, 256, size=(50, 3)) / 255.0
    faces = np.array([[0, 1, 2], [3, 4, 5]])
    path = str(tmp_path / 'w.ply')
    write_ply(verts, colors, faces, path, backend='numpy')
    got = read_ply(path, backend='numpy')
    assert list(got) == ['x', 'y', 'z', 'red', 'green', 'blue']
    printed = np.array([[float('%f' % v) for v in row] for row in verts], dtype=np.float32)
    assert np.stack([got['x'], got['y'], got['z']], 1).tobytes() == printed.tobytes()
    assert got['red'].dtype == np.uint8
    assert np.array_equal(np.stack([got['red'], got['green'], got['blue']], 1), (colors * 255).astype(np.int64))


def test_read_ply_error_cases(tmp_path):
    props, rows, faces = cc.scannet_rows()
    path = tmp_path / 'bad.ply'
    path.write_bytes(cc.ply_bytes('ascii', props, rows, faces, face_first=True))
    with pytest.raises(ValueError, match='not the first element'):
        read_ply(str(path))
    head = b'ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty list uchar int idx\nend_header\n1 0\n'
    path.write_bytes(head)
    with pytest.raises(ValueError, match='list property'):
        read_ply(str(path))
    for fmt in ('ascii', 'binary_little_endian'):
        whole = cc.ply_bytes(fmt, props, rows)
        body = whole.index(b'end_header\n') + 11
        path.write_bytes(whole[:body + (len(whole) - body) // 2])
        with pytest.raises(ValueError, match='truncated'):
            read_ply(str(path), backend='numpy')
    path.write_bytes(b'plx\n')
    with pytest.raises(ValueError, match='not a PLY'):
        read_ply(str(path))


# ---- read_cloud -----------------------------------------------------------------------------------------------------
def room(n=40, seed=3):
    rng = np.random.default_rng(seed)
    xyz = np.round(rng.uniform(-9, 9, size=(n, 3)), 3)
    rgb = rng.integers(0, 256, size=(n, 3)).astype(np.float64)
    sem = rng.integers(0, 13, size=n).astype(np.float64)
    inst = rng.integers(-1, 20, size=n).astype(np.float64)
    return xyz, rgb, sem, inst


def test_read_cloud_columns_and_rgb_modes(tmp_path):
    xyz, rgb, sem, inst = room()
    path = str(tmp_path / 'room.txt')
    np.savetxt(path, np.concatenate([xyz, rgb], 1), fmt='%.3f %.3f %.3f %d %d %d')
    info = {}
    c = read_cloud(path, backend='numpy', info=info)
    assert info['format'] == 'table' and info['backend'] == 'numpy'
    assert sorted(c) == ['rgb', 'xyz'] and c['xyz'].dtype == np.float32 and c['rgb'].dtype == np.float32
    assert c['xyz'].tobytes() == xyz.astype(np.float32).tobytes()
    assert c['rgb'].tobytes() == (rgb / 127.5 - 1).astype(np.float32).tobytes()
    assert read_cloud(path, rgb='raw', backend='numpy')['rgb'].tobytes() == rgb.astype(np.float32).tobytes()
    # labels, a dropped column, a free column, another order
    path = str(tmp_path / 'tile.xyz')
    table = np.concatenate([rgb, xyz, sem[:, None], inst[:, None], xyz[:, :1] * 2, sem[:, None]], 1)
    np.savetxt(path, table, fmt='%.6f', header='r g b x y z s i w junk', comments='// ')
    c = read_cloud(path, columns=('r', 'g', 'b', 'x', 'y', 'z', 'semantic', 'instance', 'weight', '_'), comment='/',
                   backend='numpy')
    assert sorted(c) == ['instance_labels', 'rgb', 'semantic_labels', 'weight', 'xyz']
    assert c['semantic_labels'].dtype == np.int64 and np.array_equal(c['semantic_labels'], sem.astype(np.int64))
    assert np.array_equal(c['instance_labels'], inst.astype(np.int64))
    assert c['weight'].dtype == np.float64 and c['weight'].tobytes() == (xyz[:, 0] * 2).tobytes()
    assert c['xyz'].tobytes() == xyz.astype(np.float32).tobytes()
    c = read_cloud(path, columns=('_', None, '_', 'x', 'y', 'z', '_', '_', '_', '_'), skip_lines=1, backend='numpy')
    assert sorted(c) == ['xyz']
    with pytest.raises(ValueError, match='not finite or not integral'):
        read_cloud(path, columns=('r', 'g', 'b', 'semantic', 'y', 'z', 'x', '_', '_', '_'), skip_lines=1, backend='numpy')
    with pytest.raises(ValueError, match="'x', 'y' and 'z'"):
        read_cloud(path, columns=('r', 'g', 'b', 'a', 'y', 'z', 'c', '_', '_', '_'), skip_lines=1, backend='numpy')
    with pytest.raises(ValueError, match='line 2'):
        read_cloud(path, columns=('x', 'y', 'z'), skip_lines=1, backend='numpy')


def test_read_cloud_suffix_dispatch(tmp_path):
    xyz, rgb, sem, inst = room()
    csv = str(tmp_path / 'tile.csv')
    np.savetxt(csv, np.concatenate([xyz, rgb, sem[:, None], inst[:, None]], 1), fmt='%.6f', delimiter=',')
    info = {}
    c = read_cloud(csv, columns=('x', 'y', 'z', 'r', 'g', 'b', 'semantic', 'instance'), backend='numpy', info=info)
    assert info['format'] == 'csv' and c['xyz'].tobytes() == xyz.astype(np.float32).tobytes()
    assert np.array_equal(c['instance_labels'], inst.astype(np.int64))
    semi = str(tmp_path / 'semi.csv')
    np.savetxt(semi, xyz, fmt='%.3f', delimiter=';')
    assert read_cloud(semi, columns=('x', 'y', 'z'), delimiter=';', backend='numpy')['xyz'].tobytes() == \
        xyz.astype(np.float32).tobytes()
    assert read_table(semi, delimiter=';', backend='numpy').tobytes() == xyz.tobytes()
    # KITTI
    pts = np.random.default_rng(1).normal(size=(33, 4)).astype(np.float32)
    binf = str(tmp_path / '000000.bin')
    pts.tofile(binf)
    c = read_cloud(binf, backend='numpy')
    assert sorted(c) == ['intensity', 'xyz'] and c['xyz'].tobytes() == pts[:, :3].tobytes()
    assert c['intensity'].dtype == np.float32 and c['intensity'].tobytes() == pts[:, 3].tobytes()
    # PLY, both layouts
    for label in (False, True):
        props, rows, faces = cc.scannet_rows(label=label)
        ply = str(tmp_path / f'scene{int(label)}.ply')
        open(ply, 'wb').write(cc.ply_bytes('binary_little_endian', props, rows, faces))
        c = read_cloud(ply, backend='numpy')
        assert sorted(c) == sorted(['alpha', 'rgb', 'xyz'] + (['semantic_labels'] if label else []))
        assert c['xyz'].tobytes() == np.array([r[:3] for r in rows], dtype=np.float32).tobytes()
        want = (np.array([r[3:6] for r in rows], dtype=np.float64) / 127.5 - 1).astype(np.float32)
        assert c['rgb'].tobytes() == want.tobytes()
        if label:
            assert c['semantic_labels'].dtype == np.int64 and c['semantic_labels'].tolist() == [r[7] for r in rows]
    # an explicit format wins over the suffix
    assert read_cloud(csv, format='table', columns=('x',) * 0 + ('x', 'y', 'z', 'r', 'g', 'b', 'semantic', 'instance'),
                      delimiter=',', backend='numpy')['xyz'].shape == (40, 3)


def test_read_cloud_tool_round_trip(tmp_path):
    xyz, rgb, sem, inst = room()
    path = str(tmp_path / 'room.txt')
    np.savetxt(path, np.concatenate([xyz, rgb, sem[:, None], inst[:, None]], 1), fmt='%.3f %.3f %.3f %d %d %d %d %d')
    out = str(tmp_path / 'room.pth')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'read_cloud.py'), path, '--columns', 'x', 'y', 'z', 'r',
                        'g', 'b', 'semantic', 'instance', '--backend', 'numpy', '--out', out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert '40 points' in r.stdout and 'parsed by numpy' in r.stdout and 'bounding box' in r.stdout
    got = torch.load(out, weights_only=False)
    assert len(got) == 4
    assert got[0].tobytes() == xyz.astype(np.float32).tobytes()
    assert got[1].tobytes() == (rgb / 127.5 - 1).astype(np.float32).tobytes()
    assert np.array_equal(got[2], sem.astype(np.int64)) and np.array_equal(got[3], inst.astype(np.int64))
