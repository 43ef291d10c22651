"""softgroup_amd.util.results with backend='device' (result_io.hip) against the trees the reference wrote
(tests/golden/save_results_golden.json), every C ABI entry on its own through ctypes, round trips at the size
of a scan, one scan through the real model, and bad arguments.  Equality of bytes and integers throughout."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from softgroup_amd import _lib as L  # noqa: E402
from softgroup_amd import synthetic  # noqa: E402
from softgroup_amd.util import results as R  # noqa: E402
from softgroup_amd.util.rle import rle_encode  # noqa: E402
from test_save_results import CASES, check_case, sc  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def runs_of(masks):
    """sg_instance_runs' layout (int32 starts, exclusive ends, int64 bounds) of dense masks [n_inst, length]"""
    starts, ends, bounds = [], [], [0]
    for m in masks:
        p = np.concatenate([[0], m, [0]]).astype(np.int8)
        e = np.flatnonzero(p[1:] != p[:-1])
        starts += e[0::2].tolist()
        ends += e[1::2].tolist()
        bounds.append(len(starts))
    return np.array(starts, np.int32), np.array(ends, np.int32), np.array(bounds, np.int64)


def bit_rows(masks):
    n_inst, length = masks.shape
    words = (length + 31) // 32
    padded = np.zeros((n_inst, words * 32), np.uint8)
    padded[:, :length] = masks
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder='little')).view(np.uint32).reshape(n_inst, words)


def text_from_runs(masks, first=0, count=None):
    n_inst, length = masks.shape
    count = n_inst - first if count is None else count
    s, e, b = runs_of(masks)
    text = torch.full((max(count * length * 2, 16), ), 7, dtype=torch.uint8, device='cuda')
    sd, ed, bd = dev(s), dev(e), dev(b)
    L.check(L.lib().sg_mask_text_runs(L.ptr(sd), L.ptr(ed), L.ptr(bd), len(s), n_inst, length, first, count,
                                      L.ptr(text), text.numel(), L.stream()), 'sg_mask_text_runs')
    return text[:count * length * 2].cpu().numpy().tobytes()


def text_from_bits(masks, first=0, count=None):
    n_inst, length = masks.shape
    count = n_inst - first if count is None else count
    bits = dev(bit_rows(masks).view(np.int32))
    text = torch.full((max(count * length * 2, 16), ), 7, dtype=torch.uint8, device='cuda')
    L.check(L.lib().sg_mask_text_bits(L.ptr(bits), n_inst, length, first, count, L.ptr(text), text.numel(),
                                      L.stream()), 'sg_mask_text_bits')
    return text[:count * length * 2].cpu().numpy().tobytes()


def savetxt_bytes(v, tmp_path, name='ref.txt'):
    p = tmp_path / name
    np.savetxt(str(p), v, fmt='%d')
    return p.read_bytes()


def dense_text(masks):
    return (np.stack([masks + 48, np.full_like(masks, 10)], axis=-1)).astype(np.uint8).tobytes()


def decimal_lines(v, table=None, cap=None):
    lib = L.lib()
    n = len(v)
    cap = 21 * n if cap is None else cap
    vd = dev(v, np.int64)
    td = None if table is None else dev(table, np.int32)
    text = torch.empty(max(cap, 16), dtype=torch.uint8, device='cuda')
    meta = torch.full((3, ), -1, dtype=torch.int64, device='cuda')
    ws = L.workspace(lib.sg_decimal_lines_workspace_bytes(n), 'cuda')
    L.check(lib.sg_decimal_lines(L.ptr(vd), n, L.ptr(td), 0 if table is None else len(table), L.ptr(text), cap,
                                 L.ptr(meta), L.ptr(ws), ws.numel(), L.stream()), 'sg_decimal_lines')
    total, bad, dropped = meta.cpu().tolist()
    return text[:total].cpu().numpy().tobytes(), bad, dropped


def parse_lines(data):
    lib = L.lib()
    n = len(data)
    text = dev(np.frombuffer(data, np.uint8)) if n else torch.empty(16, dtype=torch.uint8, device='cuda')
    cap = n // 2 + 1
    values = torch.empty(cap, dtype=torch.int64, device='cuda')
    meta = torch.full((2, ), -1, dtype=torch.int64, device='cuda')
    ws = L.workspace(lib.sg_parse_decimal_lines_workspace_bytes(n), 'cuda')
    L.check(lib.sg_parse_decimal_lines(L.ptr(text), n, L.ptr(values), cap, L.ptr(meta), L.ptr(ws), ws.numel(),
                                       L.stream()), 'sg_parse_decimal_lines')
    lines, bad = meta.cpu().tolist()
    return values[:lines].cpu().numpy(), bad


def parse_mask(data):
    n = len(data)
    pts = (n + 1) // 2
    text = dev(np.frombuffer(data, np.uint8)) if n else torch.empty(16, dtype=torch.uint8, device='cuda')
    flags = torch.full((max(pts, 1), ), 9, dtype=torch.uint8, device='cuda')
    bits = torch.zeros((pts + 31) // 32 + 1, dtype=torch.int32, device='cuda')
    meta = torch.full((2, ), -1, dtype=torch.int64, device='cuda')
    L.check(L.lib().sg_parse_mask_text(L.ptr(text), n, L.ptr(flags), L.ptr(bits), L.ptr(meta), L.stream()),
            'sg_parse_mask_text')
    got_pts, bad = meta.cpu().tolist()
    if n:
        assert got_pts == pts
    return flags[:pts].cpu().numpy(), bits[:(pts + 31) // 32].cpu().numpy().view(np.uint32), bad


# ---- the golden trees ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_device_backend_matches_reference_tree(name, tmp_path):
    check_case(name, str(tmp_path), 'device')


def test_device_readers_return_the_inputs(tmp_path):
    root = str(tmp_path)
    R.save_pred_instances(root, 'p', *CASES['pred_scannet']['args'], backend='device')
    scan_ids, insts, _ = CASES['pred_scannet']['args']
    dense = sc.masks('pred_scannet')
    for scan_id, scan in zip(scan_ids, insts):
        got = R.load_pred_instances(os.path.join(root, 'p'), scan_id, backend='device')
        assert len(got) == len(scan)
        for g, inst, m in zip(got, scan, dense[scan_id]):
            assert g['pred_mask'].dtype == bool and np.array_equal(g['pred_mask'], m.astype(bool))
            assert rle_encode(g['pred_mask']) == inst['pred_mask']
    R.save_gt_instances(root, 'g', *CASES['lines']['args'], backend='device')
    for scan_id, v in zip(*CASES['lines']['args'][:2]):
        got = R.read_int_lines(os.path.join(root, 'g', f'{scan_id}.txt'), backend='device')
        assert got.dtype == np.int64 and np.array_equal(got, v)
    p = tmp_path / 'odd.txt'
    p.write_bytes(b'0 1\r\n 2\n\n0\n+1')                 # (neither kernel accepts it: the split() path)
    assert R.read_mask(str(p), backend='device').tolist() == [False, True, True, False, True]
    assert R.read_int_lines(str(p), backend='device').tolist() == [0, 1, 2, 0, 1]


# ---- the entries on their own --------------------------------------------------------------------------------
@pytest.mark.parametrize('n_inst,length', [(5, 4099), (3, 4992), (7, 1), (40, 3), (9, 17), (2, 64), (1, 8), (4, 33)])
def test_mask_text_entries_agree_and_ranges_slice(n_inst, length):
    rng = np.random.default_rng(n_inst * 7919 + length)
    masks = (rng.random((n_inst, length)) < 0.4).astype(np.uint8)
    masks[0] = 0
    masks[-1] = 1
    if n_inst > 2:
        masks[1] = 0
        masks[1, [0, length - 1]] = 1
    want = dense_text(masks)
    full = text_from_runs(masks)
    assert full == want
    assert text_from_bits(masks) == want
    row = 2 * length
    for first, count in [(0, 1), (n_inst - 1, 1), (n_inst // 2, n_inst - n_inst // 2), (1, max(n_inst - 2, 0)), (0, 0),
                         (n_inst, 0)]:
        if first + count > n_inst:
            continue
        assert text_from_runs(masks, first, count) == full[first * row:(first + count) * row]
        assert text_from_bits(masks, first, count) == full[first * row:(first + count) * row]


def test_mask_text_special_masks():
    n = 4099
    masks = np.stack(sc._special_masks(n))
    assert text_from_runs(masks) == dense_text(masks)
    assert text_from_bits(masks) == dense_text(masks)


def test_mask_text_no_instances():
    masks = np.zeros((0, 100), np.uint8)
    assert text_from_runs(masks) == b'' and text_from_bits(np.zeros((0, 100), np.uint8)) == b''


def test_decimal_lines_entry(tmp_path):
    v = np.concatenate([sc._powers(), np.random.default_rng(1).integers(-2**63, 2**63 - 1, size=3000),
                        np.random.default_rng(2).integers(-99999, 99999, size=3000)])
    text, bad, dropped = decimal_lines(v)
    assert (bad, dropped) == (0, 0) and text == savetxt_bytes(v, tmp_path)
    assert decimal_lines(np.zeros(0, np.int64)) == (b'', 0, 0)
    assert decimal_lines(np.array([-7], np.int64)) == (b'-7\n', 0, 0)
    # a buffer that is too small drops lines and says so; nothing is written past it
    text, bad, dropped = decimal_lines(np.array([1, 22, 333, 4444], np.int64), cap=9)
    assert bad == 0 and dropped == 1 and text[:9] == b'1\n22\n333\n'


def test_decimal_lines_with_nyu_table(tmp_path):
    v = np.concatenate([CASES['gt_scannet']['args'][1][0], [0, 7, 999, 1000, 18999, -1, -1000, -17000]]).astype(np.int64)
    text, bad, dropped = decimal_lines(v, sc.NYU_ID)
    assert (bad, dropped) == (0, 0)
    assert text == savetxt_bytes(R._remap_nyu(v.copy(), sc.NYU_ID), tmp_path)
    # semantic index 19 of an 18-entry table: the reference's IndexError
    _, bad, _ = decimal_lines(np.array([1000, 19000, 19001, -19000], np.int64), sc.NYU_ID)
    assert bad == 3


def test_panoptic_words_entry():
    lib = L.lib()
    table = R._kitti_table(sc.LEARNING_MAP_INV, sc.KITTI_CLASSES)
    for n in (0, 1, 3, 4, 4097):
        words = sc._kitti_words(5, 5000)[:n]
        wd = dev(words.view(np.int32)) if n else torch.empty(4, dtype=torch.int32, device='cuda')
        out = torch.empty(max(n, 4), dtype=torch.int32, device='cuda')
        missing = torch.empty(2, dtype=torch.int64, device='cuda')
        host = (C.c_uint64 * 3)()
        lut = dev(table, np.int32)
        L.check(lib.sg_panoptic_kitti_words(L.ptr(wd), n, L.ptr(lut), len(table), L.ptr(out), L.ptr(missing),
                                            C.addressof(host), L.stream()), 'sg_panoptic_kitti_words')
        assert host[0] == 0
        if n:
            assert np.array_equal(out[:n].cpu().numpy().view(np.uint32), R._panoptic_numpy(words, table))
    words = sc._kitti_words(6, 1000)
    words[[77, 500, 900]] = [25 | (3 << 16), 20, 0xFFFF]
    wd, out = dev(words.view(np.int32)), torch.empty(1000, dtype=torch.int32, device='cuda')
    rc = lib.sg_panoptic_kitti_words(L.ptr(wd), 1000, L.ptr(lut), len(table), L.ptr(out), L.ptr(missing),
                                     C.addressof(host), L.stream())
    assert rc < 0 and b'sg_panoptic_kitti_words' in lib.sg_last_error()
    assert list(host) == [3, 77, 25]


def test_parse_entries_accept_only_the_writers_format():
    v, bad = parse_lines(b'12\n-3\n0\n9223372036854775807\n-9223372036854775808\n5')
    assert bad == 0 and v.tolist() == [12, -3, 0, 2**63 - 1, -2**63, 5]
    assert parse_lines(b'')[0].size == 0
    assert parse_lines(b'7')[0].tolist() == [7] and parse_lines(b'7\n')[0].tolist() == [7]
    for text in (b'1\n\n2\n', b'1 2\n', b'+1\n', b'1\r\n', b'-\n', b'9223372036854775808\n', b'\n',
                 b'-9223372036854775809\n', b'12345678901234567890\n', b'1.0\n'):
        assert parse_lines(text)[1] > 0, text
    flags, bits, bad = parse_mask(b'1\n0\n1\n')
    assert bad == 0 and flags.tolist() == [1, 0, 1] and bits.tolist() == [5]
    assert parse_mask(b'1\n0\n1')[0].tolist() == [1, 0, 1] and parse_mask(b'1')[2] == 0
    assert parse_mask(b'')[2] == 0
    good = b'1\n' * 40
    assert parse_mask(good)[2] == 0
    for pos, c in [(0, b'2'), (1, b' '), (30, b'-'), (63, b'\r'), (64, b'x'), (79, b'0')]:
        text = good[:pos] + c + good[pos + 1:]
        assert parse_mask(text)[2] > 0, (pos, c)


# ---- at the size of a scan ---------------------------------------------------------------------------------------
def test_round_trip_at_size(tmp_path):
    rng = np.random.default_rng(3)
    n_inst, length = 100, 150000
    masks = np.zeros((n_inst, length), np.uint8)
    for m in masks:
        for _ in range(int(rng.integers(1, 200))):
            lo = int(rng.integers(0, length))
            m[lo:lo + int(rng.integers(1, 3000))] = 1
    insts = [dict(scan_id='big', label_id=k % 18 + 1, conf=0.5, pred_mask=rle_encode(m)) for k, m in enumerate(masks)]
    R.save_pred_instances(str(tmp_path), 'p', ['big'], [insts], backend='device')
    got = R.load_pred_instances(str(tmp_path / 'p'), 'big', backend='device')
    assert len(got) == n_inst
    for g, m in zip(got, masks):
        assert np.array_equal(g['pred_mask'], m.astype(bool))
    assert (tmp_path / 'p' / 'predicted_masks' / 'big_037.txt').read_bytes() == savetxt_bytes(masks[37], tmp_path)
    # the bit-row entry on the same masks, and the reader's bit rows
    assert text_from_bits(masks[:8]) == dense_text(masks[:8])
    flags, bits, bad = parse_mask(dense_text(masks[5:6]))
    assert bad == 0 and np.array_equal(flags, masks[5]) and np.array_equal(bits, bit_rows(masks[5:6])[0])
    v = rng.integers(-2**40, 2**40, size=600000)
    v[:1000] = rng.integers(-2**63, 2**63 - 1, size=1000)
    R.save_gt_instances(str(tmp_path), 'g', ['big'], [v], backend='device')
    assert np.array_equal(R.read_int_lines(str(tmp_path / 'g' / 'big.txt'), backend='device'), v)
    assert (tmp_path / 'g' / 'big.txt').read_bytes() == R._int_lines_numpy(v).tobytes()


def test_scan_through_the_model(tmp_path):
    xyz, rgb, inst = synthetic.scene_s2(seed=3, n=30000, room_scale=0.45)
    batch = synthetic.make_batch(xyz, rgb, instance_labels=inst)
    model = synthetic.build_model(seed=0)
    with torch.no_grad():
        res = model(batch)

    class Dataset:
        NYU_ID = sc.NYU_ID

    tasks = synthetic.SCANNET_MODEL_CFG['test_cfg']['eval_tasks']
    R.save_results(str(tmp_path), [res], tasks, Dataset, backend='device')
    preds = res['pred_instances']
    assert len(preds) > 0
    got = R.load_pred_instances(str(tmp_path / 'pred_instance'), res['scan_id'], backend='device')
    assert len(got) == len(preds)
    for g, p in zip(got, preds):
        assert rle_encode(g['pred_mask']) == p['pred_mask']
        assert g['label_id'] == sc.NYU_ID[p['label_id'] - 1] and g['conf'] == float(f"{p['conf']:.4f}")
    gt = R.read_int_lines(str(tmp_path / 'gt_instance' / f"{res['scan_id']}.txt"), backend='device')
    assert np.array_equal(gt, R._remap_nyu(np.asarray(res['gt_instances']).astype(np.int64), sc.NYU_ID))
    assert np.array_equal(np.load(str(tmp_path / 'semantic_pred' / f"{res['scan_id']}.npy")), res['semantic_preds'])
    assert sorted(os.listdir(str(tmp_path))) == ['colors', 'coords', 'gt_instance', 'offset_label', 'offset_pred',
                                                 'pred_instance', 'semantic_label', 'semantic_pred']


# ---- bad arguments: a negative status that names the entry, no launch ------------------------------------------------
def test_bad_arguments():
    lib = L.lib()
    buf = torch.zeros(256, dtype=torch.uint8, device='cuda')
    p, s = L.ptr(buf), L.stream()

    def refused(rc, name):
        assert rc < 0 and name.encode() in lib.sg_last_error(), name

    refused(lib.sg_mask_text_runs(p, p, p, 0, 2, 8, 1, 2, p, 256, s), 'sg_mask_text_runs')          # range past n_inst
    refused(lib.sg_mask_text_runs(p, p, p, 0, 2, 8, 0, 2, p, 31, s), 'sg_mask_text_runs')           # buffer too small
    refused(lib.sg_mask_text_runs(p, p, p, 0, 2, 8, 0, 2, p + 4, 200, s), 'sg_mask_text_runs')      # alignment
    refused(lib.sg_mask_text_runs(p, p, None, 0, 2, 8, 0, 2, p, 256, s), 'sg_mask_text_runs')
    refused(lib.sg_mask_text_bits(None, 2, 8, 0, 2, p, 256, s), 'sg_mask_text_bits')
    refused(lib.sg_mask_text_bits(p, 2, -1, 0, 2, p, 256, s), 'sg_mask_text_bits')
    refused(lib.sg_decimal_lines(p, -1, None, 0, p, 256, p, p, 256, s), 'sg_decimal_lines')
    refused(lib.sg_decimal_lines(p, 4, None, 0, p, 256, p, p, 16, s), 'sg_decimal_lines')           # workspace
    refused(lib.sg_decimal_lines(p, 4, p, 0, p, 256, p, p, 256, s), 'sg_decimal_lines')             # empty table
    host = (C.c_uint64 * 3)()
    refused(lib.sg_panoptic_kitti_words(p, 4, None, 20, p, p, C.addressof(host), s), 'sg_panoptic_kitti_words')
    refused(lib.sg_panoptic_kitti_words(p, 4, p, 70000, p, p, C.addressof(host), s), 'sg_panoptic_kitti_words')
    refused(lib.sg_parse_decimal_lines(None, 8, p, 8, p, p, 256, s), 'sg_parse_decimal_lines')
    refused(lib.sg_parse_decimal_lines(p, 8, p, 8, p, p, 0, s), 'sg_parse_decimal_lines')
    refused(lib.sg_parse_mask_text(p + 1, 8, p, None, p, s), 'sg_parse_mask_text')
    refused(lib.sg_parse_mask_text(p, -2, p, None, p, s), 'sg_parse_mask_text')
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0
