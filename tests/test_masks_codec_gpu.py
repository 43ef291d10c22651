"""The mask-list codec of ``softgroup_amd.util.masks`` on the device: RLE text -> ``sg_inst_rle_parse`` ->
``sg_mask_bits_from_runs`` against ``packed_rows``, the two check flags, and bit rows / runs ->
``sg_rle_format_device`` against ``rle_encode``, at the word and byte boundaries of a row.  Equality everywhere."""
import os
import sys

import numpy as np
import pytest
import torch

from softgroup_amd.ops import resample as RS
from softgroup_amd.util import masks as M
from softgroup_amd.util import rle_encode

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_masks_codec import N_POINTS, dense_masks, insts_of  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)


def lists_of(n):
    """all-RLE lists of 1, 2 and 5 masks: an empty mask alone, first, in the middle and last"""
    empty, full, first, last, r0, r1 = (rle_encode(d) for d in dense_masks(n))
    return [[r0], [empty], [empty, r0], [r1, empty], [empty, r0, full, r1, last], [r0, first, empty, r1, full],
            [last, r1, r0, first, empty], [empty] * 5]


def host_bytes(bits):
    return bits.cpu().numpy().view(np.uint8)


@pytest.mark.parametrize('n', N_POINTS)
def test_rows_device_of_rle_lists_equals_packed_rows(n):
    for masks in lists_of(n):
        insts = insts_of(masks)
        bits, check = M.rows_device(insts, n, DEV)
        assert bits.dtype == torch.int32 and tuple(bits.shape) == (len(insts), (n + 31) // 32) and bits.device == DEV
        assert np.array_equal(host_bytes(bits), M.packed_rows(insts, n))
        assert check.device == DEV and check.cpu().tolist() == [0, 0]
        assert torch.equal(M.checked_rows_device(insts, n, DEV), bits)


@pytest.mark.parametrize('n', N_POINTS)
def test_rows_device_with_a_dense_entry_packs_on_the_host(n):
    dense = dense_masks(n)
    masks = [rle_encode(d) for d in dense]
    masks[3] = dense[3].astype(bool)
    insts = insts_of(masks)
    bits, check = M.rows_device(insts, n, DEV)
    assert check is None and bits.dtype == torch.int32 and bits.device == DEV
    assert np.array_equal(host_bytes(bits), M.packed_rows(insts, n))
    assert torch.equal(M.checked_rows_device(insts, n, DEV), bits)


@pytest.mark.parametrize('text', ('1 2 a 1', '1 2 5', '1 2 40 3'))
def test_malformed_text_raises_value_error(text):
    """a letter, an odd token count, a run outside the mask"""
    insts = insts_of([dict(length=33, counts='3 4'), dict(length=33, counts=text)])
    with pytest.raises(ValueError, match='malformed RLE text') as e:
        M.checked_rows_device(insts, 33, DEV)
    assert not isinstance(e.value, M.UnsortedRuns)
    assert M.rows_device(insts, 33, DEV)[1].cpu().tolist()[0]


def test_descending_runs_inside_a_mask_raise_and_across_masks_do_not():
    n = 65
    inside = insts_of([dict(length=n, counts='1 2'), dict(length=n, counts='40 5 3 4')])
    with pytest.raises(M.UnsortedRuns, match="use backend='numpy'"):
        M.checked_rows_device(inside, n, DEV)
    assert M.rows_device(inside, n, DEV)[1].cpu().tolist() == [0, 1]
    overlap = insts_of([dict(length=n, counts='3 10 5 2')])
    with pytest.raises(M.UnsortedRuns):
        M.checked_rows_device(overlap, n, DEV)
    # mask 1 starts below where mask 0 ended: the order inside every mask is what counts
    across = insts_of([dict(length=n, counts='40 5 60 6'), dict(length=n, counts='3 4 33 2'),
                       dict(length=n, counts=''), dict(length=n, counts='1 1')])
    bits, check = M.rows_device(across, n, DEV)
    assert check.cpu().tolist() == [0, 0]
    assert np.array_equal(host_bytes(bits), M.packed_rows(across, n))
    assert torch.equal(M.checked_rows_device(across, n, DEV), bits)


@pytest.mark.parametrize('n', N_POINTS)
def test_round_trip_is_rle_encode(n):
    for masks in lists_of(n):
        insts = insts_of(masks)
        bits, _ = M.rows_device(insts, n, DEV)
        assert M.rle_dicts_from_bits_device(bits, n, DEV) == masks
        starts, ends, bounds = RS.mask_runs_from_bits(bits, n)
        extra = torch.tensor([7], dtype=torch.int32, device=DEV)
        got, back = M.rle_dicts_from_runs_device(starts, ends, bounds, len(insts), n, DEV, extra=extra)
        assert got == masks and back == [7] and extra.cpu().tolist() == [7]


def test_no_runs_at_all_gives_empty_strings():
    starts = torch.empty(1, dtype=torch.int32, device=DEV)[:0]      # (what mask_runs_from_bits returns for no runs)
    ends = torch.empty(1, dtype=torch.int32, device=DEV)[:0]
    bounds = torch.zeros(4, dtype=torch.int64, device=DEV)
    got = M.rle_dicts_from_runs_device(starts, ends, bounds, 3, 65, DEV)
    assert got == [dict(length=65, counts='')] * 3
