"""cloud_io.hip on the GPU: sg_text_table_count / sg_text_table_parse against parse_table_numpy (the definition).  The
only tolerated difference between the two backends is none: values and row lines are compared as bytes, exceptions
by their text.  Sizes cross the launch cap of 524 288 threads and the scan's single-level form at 4 194 304 bytes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_io_cases as cc  # noqa: E402

from softgroup_amd.ops import text as T  # noqa: E402
from softgroup_amd.util import read_cloud, read_ply, read_table, write_ply  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64


def both(data, **kw):
    """(values, lines) of the device backend after checking them against the definition, byte for byte"""
    ref, ref_lines = T.parse_table_numpy(data, return_lines=True, **kw)
    info = {}
    got, lines = T.parse_table(data, backend='device', return_lines=True, info=info, **kw)
    assert info['backend'] == 'device'
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == ref.shape
    assert got.view(np.uint8).tobytes() == ref.view(np.uint8).tobytes()
    assert lines.dtype == np.int32 and lines.tobytes() == ref_lines.tobytes()
    return got, lines, info


@pytest.mark.parametrize('case', cc.grammar_files(), ids=lambda c: c[0])
def test_grammar_files_on_the_device(case):
    name, data, kw, bad_line = case
    if bad_line is not None:
        with pytest.raises(ValueError) as want:
            T.parse_table_numpy(data, **kw)
        with pytest.raises(ValueError) as got:
            T.parse_table(data, backend='device', **kw)
        assert str(got.value) == str(want.value) and f'line {bad_line}' in str(got.value)
        return
    got, lines, info = both(data, **kw)
    as32 = T.parse_table(data, backend='device', dtype=np.float32, **kw)
    assert as32.dtype == np.float32 and as32.tobytes() == got.astype(np.float32).tobytes()
    if len(data):
        dev = T.parse_table(torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda(), backend='device', **kw)
        assert dev.is_cuda and dev.dtype == torch.float64 and dev.cpu().numpy().tobytes() == got.tobytes()


def test_every_spelling_is_converted_on_the_device():
    data = cc.spelling_table(rows=4000, cols=6)
    got, lines, info = both(data, cols=6)
    assert got.shape == (4000, 6) and info['declined'] == 0


def poisoned(rows, cols):
    """values / row_status / row_line with GUARD sentinel elements on both sides: (whole buffers, the views inside)"""
    whole = (torch.full((rows * cols + 2 * GUARD,), float('nan'), dtype=torch.float64, device='cuda'),
             torch.full((rows + 2 * GUARD,), 0xA5, dtype=torch.uint8, device='cuda'),
             torch.full((rows + 2 * GUARD,), -77, dtype=torch.int32, device='cuda'))
    whole[0].view(torch.int64).fill_(0x7FF8DEADBEEF0001)
    views = (whole[0][GUARD:GUARD + rows * cols].view(rows, cols), whole[1][GUARD:GUARD + rows],
             whole[2][GUARD:GUARD + rows])
    return whole, views


def guards_intact(whole, rows, cols):
    v, s, ln = whole
    poison = torch.tensor(0x7FF8DEADBEEF0001, dtype=torch.int64, device='cuda')
    ends = torch.cat([v[:GUARD], v[GUARD + rows * cols:]]).view(torch.int64)
    return bool((ends == poison).all()) and bool((torch.cat([s[:GUARD], s[GUARD + rows:]]) == 0xA5).all()) and \
        bool((torch.cat([ln[:GUARD], ln[GUARD + rows:]]) == -77).all())


def test_declined_fields_are_left_to_the_host():
    data, which = cc.declined_table(rows=700, cols=6)
    got, lines, info = both(data, cols=6)
    assert info['declined'] == len(which) == 100
    # the kernel alone: exactly those rows carry bit 0, their declined slot keeps the poison, the rest is converted
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    whole, (values, status, row_line) = poisoned(700, 6)
    _, _, _, meta = T.table_parse_device(text, 6, 700, values=values, row_status=status, row_line=row_line)
    assert meta[:7] == [700, 700, 0, len(which), 0, 2**63 - 1, 0]
    assert torch.nonzero(status).flatten().tolist() == which and set(status[which].tolist()) == {1}
    raw = values.cpu().numpy().view(np.int64)
    untouched = raw == 0x7FF8DEADBEEF0001
    assert untouched.sum() == len(which) and untouched[which].sum(1).tolist() == [1] * len(which)
    assert np.array_equal(raw[~untouched], got.view(np.int64)[~untouched])
    assert row_line.cpu().numpy().tobytes() == lines.tobytes()
    assert guards_intact(whole, 700, 6)


def test_more_rows_than_one_launch():
    data = b'1 2\n' * 530000
    got, lines, info = both(data)
    assert got.shape == (530000, 2) and info['declined'] == 0
    assert lines[0] == 1 and lines[-1] == 530000


def test_text_above_the_single_level_scan():
    rng = np.random.default_rng(21)
    x = rng.uniform(-300, 300, size=(100000, 6))
    data = '\n'.join(' '.join('%.8f' % v for v in row) for row in x.tolist()).encode()      # (no last newline)
    assert len(data) >= 4300000
    got, lines, info = both(data, cols=6)
    assert got.shape == (100000, 6) and info['declined'] == 0
    assert T.table_count_device(torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()) == (100000, 100000, 0)


def test_rows_at_every_offset():
    data = cc.offsets_table()
    got, lines, info = both(data, cols=1)
    assert got.shape == (256, 1)
    starts = np.concatenate(([0], np.flatnonzero(np.frombuffer(data, dtype=np.uint8) == 10)[:-1] + 1))
    assert set((starts % 16).tolist()) == set(range(16))


def test_guards_well_formed_and_wrong_row_counts():
    data = cc.spelling_table(rows=500, cols=6)
    ref = T.parse_table_numpy(data)
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    whole, (values, status, row_line) = poisoned(500, 6)
    _, _, _, meta = T.table_parse_device(text, 6, 500, values=values, row_status=status, row_line=row_line)
    assert meta[1] == 500 and meta[3:7] == [0, 0, 2**63 - 1, 0]
    assert values.cpu().numpy().tobytes() == ref.tobytes() and not status.any()
    assert guards_intact(whole, 500, 6)
    for rows in (499, 501):
        whole, (values, status, row_line) = poisoned(rows, 6)
        _, _, _, meta = T.table_parse_device(text, 6, rows, values=values, row_status=status, row_line=row_line)
        assert meta[1] == 500 and meta[6] == 1, meta
        assert guards_intact(whole, rows, 6)
        assert values[:499].cpu().numpy().tobytes() == ref[:499].tobytes()
        if rows == 501:      # one row more than the text holds: the last row of the arrays is not written
            assert int(status[500]) == 0xA5 and int(row_line[500]) == -77


@pytest.mark.parametrize('fields', [3, 70])
def test_guards_ragged_rows(fields):
    good = ' '.join(['1.5'] * 6)
    lines = [good] * 40
    for k in (7, 8, 31):
        lines[k] = ' '.join(['2.5'] * fields)
    data = ('\n'.join(lines) + '\n').encode()
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    whole, (values, status, row_line) = poisoned(40, 6)
    _, _, _, meta = T.table_parse_device(text, 6, 40, values=values, row_status=status, row_line=row_line)
    assert meta[:7] == [40, 40, 0, 0, 3, 8, 0]
    assert torch.nonzero(status).flatten().tolist() == [7, 8, 31] and set(status[[7, 8, 31]].tolist()) == {2}
    assert guards_intact(whole, 40, 6)
    keep = [k for k in range(40) if k not in (7, 8, 31)]
    assert (values[keep] == 1.5).all()
    with pytest.raises(ValueError, match='line 8'):
        T.parse_table(data, cols=6, backend='device')


def test_guards_long_token():
    for n, bad in ((64, False), (65, True)):
        data = ('1 2\n' + '0' * (n - 1) + '7 2\n3 4\n').encode()
        text = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        whole, (values, status, row_line) = poisoned(3, 2)
        _, _, _, meta = T.table_parse_device(text, 2, 3, values=values, row_status=status, row_line=row_line)
        assert meta[:7] == [3, 3, 0, 0, int(bad), 2 if bad else 2**63 - 1, 0]
        assert status.tolist() == [0, 2 if bad else 0, 0]
        assert guards_intact(whole, 3, 2)
        if not bad:
            assert values.tolist() == [[1.0, 2.0], [7.0, 2.0], [3.0, 4.0]]


def test_read_ply_and_read_cloud_on_the_device(tmp_path):
    for label in (False, True):
        props, rows, faces = cc.scannet_rows(n=301, label=label)
        path = str(tmp_path / f'scene{int(label)}.ply')
        open(path, 'wb').write(cc.ply_bytes('ascii', props, rows, faces))
        want, got = read_ply(path, backend='numpy'), read_ply(path, backend='device')
        assert list(got) == list(want)
        for k in want:
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    rng = np.random.default_rng(0)
    written = str(tmp_path / 'written.ply')
    write_ply(rng.uniform(-3, 3, size=(999, 3)).astype(np.float32), rng.uniform(0, 1, size=(999, 3)),
              np.array([[0, 1, 2]]), written, backend='numpy')
    room = str(tmp_path / 'room.txt')
    table = np.concatenate([rng.uniform(-9, 9, size=(2000, 3)), rng.integers(0, 256, size=(2000, 3)),
                            rng.integers(0, 13, size=(2000, 2))], 1)
    np.savetxt(room, table, fmt='%.3f %.3f %.3f %d %d %d %d %d')
    tile = str(tmp_path / 'tile.csv')
    np.savetxt(tile, table, fmt='%.6f', delimiter=',')
    kitti = str(tmp_path / '000000.bin')
    rng.normal(size=(100, 4)).astype(np.float32).tofile(kitti)
    columns = ('x', 'y', 'z', 'r', 'g', 'b', 'semantic', 'instance')
    for path, kw in ((written, {}), (path, {}), (room, dict(columns=columns)), (room, dict(columns=columns, rgb='raw')),
                     (tile, dict(columns=columns)), (kitti, {})):
        info = {}
        want, got = read_cloud(path, backend='numpy', **kw), read_cloud(path, backend='device', info=info, **kw)
        assert info['backend'] == 'device' and sorted(got) == sorted(want)
        for k in want:
            assert got[k].is_cuda and got[k].cpu().numpy().dtype == want[k].dtype, k
            assert got[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    t = read_table(room, backend='device')
    assert t.is_cuda and t.cpu().numpy().tobytes() == read_table(room, backend='numpy').tobytes()
    with pytest.raises(ValueError, match='not finite or not integral'):
        read_cloud(room, columns=('semantic', 'y', 'z', 'r', 'g', 'b', 'x', '_'), backend='device')


def test_two_device_calls_give_identical_bytes():
    data, which = cc.declined_table(rows=3000, cols=6)
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    a, la = T.parse_table(text, cols=6, backend='device', return_lines=True)
    b, lb = T.parse_table(text, cols=6, backend='device', return_lines=True)
    assert a.is_cuda and la.is_cuda
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() and la.cpu().numpy().tobytes() == lb.cpu().numpy().tobytes()
    assert a.cpu().numpy().tobytes() == T.parse_table_numpy(data).tobytes()
