"""The mask-list codec of ``softgroup_amd.util.masks`` on the host: a list of instance dicts -> packed bit rows ->
canonical RLE dicts, at the word and byte boundaries of a row.  References: ``rle_decode`` / ``rle_encode`` (the
reference's wire format) and ``np.packbits``.  Equality everywhere."""
import numpy as np
import pytest
import torch

from softgroup_amd.ops._args import choose_backend
from softgroup_amd.util import masks as M
from softgroup_amd.util import rle_decode, rle_encode

N_POINTS = (1, 31, 32, 33, 63, 64, 65)


def dense_masks(n):
    """the dense uint8 masks every test uses: empty, full, the first point, the last point, two random ones"""
    rng = np.random.default_rng(n)
    first, last = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    first[0] = last[n - 1] = 1
    return [np.zeros(n, np.uint8), np.ones(n, np.uint8), first, last, (rng.random(n) < 0.5).astype(np.uint8),
            (rng.random(n) < 0.2).astype(np.uint8)]


def want_rows(dense, n):
    rows = np.zeros((len(dense), (n + 31) // 32 * 4), np.uint8)
    for k, d in enumerate(dense):
        p = np.packbits(d, bitorder='little')
        rows[k, :p.size] = p
    return rows


def insts_of(masks):
    return [dict(scan_id='s', label_id=1 + k, conf=0.5, pred_mask=m) for k, m in enumerate(masks)]


def odd_texts(n):
    """run-length strings no encoder here writes: runs out of order, touching, overlapping, past ``length``"""
    a = max(n // 4, 1)
    return [f'{n // 2 + 1} {a} 1 {a}', f'1 {a} {a + 1} {a}', f'1 {n // 2 + 1} {n // 4 + 1} {n // 2 + 1}', f'{n} 10',
            f'{max(n - 2, 1)} 10 1 1']


@pytest.mark.parametrize('n', N_POINTS)
def test_packed_rows_of_rle_bool_and_uint8(n):
    dense = dense_masks(n)
    want = want_rows(dense, n)
    rle = [rle_encode(d) for d in dense]
    assert all(np.array_equal(rle_decode(r), d) for r, d in zip(rle, dense))
    forms = (rle, [d.astype(bool) for d in dense], dense)
    for masks in forms:
        got = M.packed_rows(insts_of(masks), n)
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
        for m, d in zip(masks, dense):
            row = M.dense_of(m, n)
            assert row.dtype == np.uint8 and np.array_equal(row, d)
    mixed = [forms[k % 3][k] for k in range(len(dense))]
    assert np.array_equal(M.packed_rows(insts_of(mixed), n), want)
    assert M.packed_rows([], n).shape == (0, want.shape[1])


@pytest.mark.parametrize('n', N_POINTS)
def test_rows_of_unsorted_text_are_what_rle_decode_paints(n):
    rle = [dict(length=n, counts=t) for t in odd_texts(n)]
    dense = [rle_decode(r) for r in rle]
    assert any(d.any() for d in dense)
    for r, d in zip(rle, dense):
        assert np.array_equal(M.dense_of(r, n), d)
    assert np.array_equal(M.packed_rows(insts_of(rle), n), want_rows(dense, n))


def test_mask_length():
    assert M.mask_length([]) is None
    assert M.mask_length(insts_of([rle_encode(np.ones(33, np.uint8)), np.zeros(33, bool)])) == 33
    with pytest.raises(ValueError, match='masks of 32 and of 33 points in one list'):
        M.mask_length(insts_of([rle_encode(np.ones(32, np.uint8)), np.zeros(33, bool)]))


@pytest.mark.parametrize('n', N_POINTS)
def test_rle_dicts_from_bits_numpy_is_rle_encode(n):
    dense = dense_masks(n)
    want = [rle_encode(d) for d in dense]
    assert want[0]['counts'] == ''
    got = M.rle_dicts_from_bits_numpy(M.packed_rows(insts_of(want), n), n)
    assert got == want and all(type(g['counts']) is str and g['length'] == n for g in got)
    # 32-bit words in, as the device stages hand them over
    assert M.rle_dicts_from_bits_numpy(M.packed_rows(insts_of(dense), n).view(np.int32), n) == want


@pytest.mark.parametrize('empty', (0, 1, 2))
def test_rle_dicts_from_runs_numpy_with_an_empty_mask(empty):
    n = 65
    runs = [[(0, 3), (31, 33)], [(64, 65)], [(5, 6), (7, 8), (32, 64)]]
    runs[empty] = []
    starts = np.array([s for r in runs for s, _ in r], np.int32)
    ends = np.array([e for r in runs for _, e in r], np.int32)
    bounds = np.cumsum([0] + [len(r) for r in runs]).astype(np.int64)
    want = []
    for r in runs:
        d = np.zeros(n, np.uint8)
        for s, e in r:
            d[s:e] = 1
        want.append(rle_encode(d))
    assert want[empty]['counts'] == ''
    assert M.rle_dicts_from_runs_numpy(starts, ends, bounds, n) == want


def test_carried_copies_the_keys_that_exist():
    mask = dict(length=3, counts='1 1')
    src = dict(scan_id='s', label_id=4, conf=0.25, pred_mask=dict(length=3, counts=''), other=1)
    out = M.carried(src, mask)
    assert out == dict(scan_id='s', label_id=4, conf=0.25, pred_mask=mask) and out['pred_mask'] is mask
    out['conf'] = 1.0
    assert src['conf'] == 0.25 and src['pred_mask'] == dict(length=3, counts='') and src['other'] == 1
    assert M.carried(dict(label_id=2, pred_mask=None), mask) == dict(label_id=2, pred_mask=mask)
    assert M.carried({}, mask) == dict(pred_mask=mask)


def test_choose_backend(monkeypatch):
    with pytest.raises(ValueError, match="backend 'gpu': one of 'auto', 'device', 'numpy'"):
        choose_backend('gpu', 'device')
    assert choose_backend('device', 'numpy') == 'device' and choose_backend('numpy', 'device') == 'numpy'
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    assert choose_backend('auto', 'device') == 'numpy'
    assert choose_backend('device', 'numpy') == 'device'
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    assert choose_backend('auto', 'device') == 'device' and choose_backend('auto', 'numpy') == 'numpy'
