"""The HIP kernels of csrc/stitch.hip and the device path of ``stitch_results``, on the inputs and against the
plain-loop references of tests/test_stitch.py: equality everywhere, two calls give equal bytes."""
import os
import sys

import numpy as np
import pytest
import torch

from softgroup_amd import _lib as L
from softgroup_amd import synthetic
from softgroup_amd.data import apply_sample, tile_cloud
from softgroup_amd.ops import stitch as ST
from softgroup_amd.util import rle_decode, stitch_results

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_stitch import (BAD_TILE_CLOUDS, E2E_CASES, EDGE_N, LINK_BITS, LINK_SHAPES, brute_components, brute_links,  # noqa: E402
                         brute_shared, brute_tiles, brute_union, check_e2e, check_tiles, e2e_case, edge_tile_cloud,
                         graph_cases, link_case, margin_only_case, packed_rows, runs_to_rle, shared_cases, tile_cases,
                         tile_reference, too_many_tiles_cloud, union_cases, union_inputs)

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared inputs are read-only)


# ---- tiles ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(tile_cases()))
def test_tile_cloud_device_equals_plain_loop(name):
    xyz, size, margin, origin = tile_cases()[name]
    ts = tile_cloud(dev(xyz), size=size, margin=margin, origin=origin, backend='device')
    assert ts.is_cuda and ts.point_ids[0].is_cuda and ts.core_pos.dtype == torch.int32
    check_tiles(ts, tile_reference(name), xyz.shape[0], full_grid=name in ('full_grid', 'single_tile'))
    again = ST.tile_assign(dev(xyz), size, margin, origin)
    assert torch.equal(again[2].long(), ts.tile_points) and torch.equal(again[4], ts.core_pos)
    twin = ST.tile_assign_numpy(xyz, size, margin, origin)
    for g, w in zip(again[:5], twin[:5]):
        assert g.cpu().numpy().dtype == w.dtype and np.array_equal(g.cpu().numpy(), w)
    assert again[5] == twin[5]


@pytest.mark.parametrize('n', EDGE_N)
def test_tile_cloud_device_edge_sizes(n):
    x = edge_tile_cloud(n)
    ts = tile_cloud(dev(x).reshape(n, 3), size=0.5, margin=0.125, origin=(0.0, 0.0), backend='device')
    check_tiles(ts, brute_tiles(x, 0.5, 0.125, (0.0, 0.0)), n)
    host = tile_cloud(x, size=0.5, margin=0.125, origin=(0.0, 0.0), backend='device')          # numpy in, numpy out
    assert isinstance(host.core_tile, np.ndarray) and np.array_equal(host.tile_points, ts.tile_points.cpu().numpy())


@pytest.mark.parametrize('name', sorted(BAD_TILE_CLOUDS))
def test_tile_cloud_device_rejects_invalid_points(name):
    x, size = BAD_TILE_CLOUDS[name]
    with pytest.raises(ValueError):
        tile_cloud(dev(x), size=size, margin=0.0, origin=(0.0, 0.0), backend='device')
    big = np.array(tile_cases()['lattice'][0])          # one invalid point among 4 000 (and among 5 000): still no result
    big[3210] = x[1]
    with pytest.raises(ValueError):
        tile_cloud(dev(big), size=size, margin=0.0, origin=(0.0, 0.0), backend='device')
    big = np.array(tile_cases()['tenth'][0])
    big[4321] = x[1]
    with pytest.raises(ValueError):
        tile_cloud(dev(big), size=size, margin=0.0, origin=(0.0, 0.0), backend='device')


def test_tile_cloud_device_rejects_too_many_tiles():
    x = too_many_tiles_cloud()
    with pytest.raises(ValueError, match='65535'):
        tile_cloud(dev(x), size=1.0, margin=0.0, origin=(0.0, 0.0), backend='device')
    ok = tile_cloud(dev(x[:65535]), size=1.0, margin=0.25, origin=(0.0, 0.0), backend='device')
    assert len(ok) == 65535 and ok.cells.cpu().numpy().tolist() == [[i % 257, i // 257] for i in range(65535)]


# ---- shared points ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(shared_cases()))
def test_tile_shared_device(name):
    a, b = shared_cases()[name]
    want = brute_shared(a, b)
    pos_a, pos_b, count = ST.tile_shared(dev(a), dev(b))
    c = int(count.item())
    assert pos_a.dtype == torch.int32 and c == len(want[0])
    assert pos_a[:c].cpu().tolist() == want[0] and pos_b[:c].cpu().tolist() == want[1]


# ---- links ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', LINK_SHAPES)
@pytest.mark.parametrize('n_bits', LINK_BITS)
def test_mask_cross_links_device(n_bits, shape):
    a, b, la, lb, pa, pb = link_case(n_bits, *shape)
    n_a, n_b = shape
    n_total = 7 + n_a + 3 + n_b
    base_a, base_b = 7, 7 + n_a + 3
    da, db = dev(pa.view(np.int32)), dev(pb.view(np.int32))
    for measure, min_shared in (('iou', 1), ('min', 1), ('iou', 3)):
        adj, inter, ca, cb = ST.mask_cross_links(da, db, n_bits, la, lb, base_a, base_b, n_total, 0.5, measure, min_shared,
                                                 return_counts=True)
        link, want_inter, want_ca, want_cb = ST.mask_cross_links_numpy(pa, pb, n_bits, la, lb, 0.5, measure, min_shared)
        assert np.array_equal(inter.cpu().numpy(), want_inter)              # garbage beyond n_bits is ignored
        assert np.array_equal(ca.cpu().numpy(), want_ca) and np.array_equal(cb.cpu().numpy(), want_cb)
        want_adj = ST.adjacency_from_edges([(base_a + i, base_b + j) for i, j in zip(*np.nonzero(link))], n_total)
        assert np.array_equal(adj.cpu().numpy().view(np.uint32), want_adj)
        if n_bits <= 2049:
            assert np.array_equal(link, brute_links(a, b, la, lb, 0.5, measure, min_shared)[0])
    again = ST.mask_cross_links(da, db, n_bits, la, lb, base_a, base_b, n_total, 0.5, 'iou', 3)
    assert torch.equal(again, adj)


# ---- components -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(graph_cases()))
def test_stitch_components_device(name):
    n, edges = graph_cases()[name]
    adj = ST.adjacency_from_edges(edges, n)
    comp = ST.stitch_components(dev(adj.view(np.int32)), n)
    assert comp.dtype == torch.int32 and comp.cpu().tolist() == brute_components(n, edges)


def test_stitch_components_device_ignores_bits_beyond_n():
    n, edges = graph_cases()['thirty_three']
    adj = ST.adjacency_from_edges(edges, n)
    adj[:, 1] |= np.uint32(0xFFFFFFFE)                  # nodes 33 .. 63 do not exist
    comp = ST.stitch_components(dev(adj.view(np.int32)), n)
    assert comp.cpu().tolist() == brute_components(n, edges)


# ---- ids and union ----------------------------------------------------------------------------------------------------
def test_mask_bits_ids_device():
    rng = np.random.default_rng(2)
    for n_bits, n in ((1001, 7), (32, 3), (9000, 5), (1, 2)):
        dense = rng.random((n, n_bits)) < 0.3
        dense[n - 1] = False
        rows = packed_rows(dense)
        if n_bits & 31:
            rows[:, (n_bits + 7) // 8:] = 0xFF          # bits at and beyond n_bits are ignored
        index_map = np.sort(rng.choice(50000, n_bits, replace=False)).astype(np.int32)
        core = (rng.random(n_bits) < 0.5).astype(np.uint8)
        want_ids, want_cnt, want_core = ST.mask_bits_ids_numpy(packed_rows(dense), n_bits, index_map, core)
        bits = dev(rows.view(np.int32))
        cnt, core_cnt = ST.mask_bits_ids_count(bits, n_bits, dev(core))
        assert np.array_equal(cnt.cpu().numpy(), want_cnt) and np.array_equal(core_cnt.cpu().numpy(), want_core)
        total = int(want_cnt.sum())
        off = np.zeros(n, np.int64)
        np.cumsum(want_cnt[:-1], out=off[1:])
        ids = torch.full((total, ), -7, dtype=torch.int32, device='cuda')
        keys = torch.full((total, ), -7, dtype=torch.int32, device='cuda')
        meta = torch.zeros(1, dtype=torch.int32, device='cuda')
        row_key = np.arange(n, dtype=np.int32) - 1                    # row 0: no object
        ST.mask_bits_ids_fill(bits, n_bits, dev(index_map), 50000, dev(off), dev(row_key), ids, keys, meta)
        assert np.array_equal(ids.cpu().numpy(), want_ids) and int(meta.item()) == 0
        want_keys = np.repeat(np.where(row_key < 0, 0xFFFF, row_key), want_cnt)
        assert np.array_equal(keys.cpu().numpy(), want_keys)
        ST.mask_bits_ids_fill(bits, n_bits, dev(index_map), int(index_map[-1]), dev(off), dev(row_key), ids, keys, meta)
        assert int(meta.item()) == (1 if dense[:, -1].any() else 0)     # a map value outside the cloud is flagged


@pytest.mark.parametrize('name', sorted(union_cases()))
def test_stitch_union_device(name):
    case = union_cases()[name]
    ids, keys = union_inputs(case)
    starts, ends, bounds = ST.stitch_union(dev(ids), dev(keys), case[1], case[0])
    want = ST.stitch_union_numpy(ids, keys, case[1], case[0])
    for g, w in zip((starts, ends, bounds), want):
        assert g.cpu().numpy().dtype == w.dtype and np.array_equal(g.cpu().numpy(), w)
    assert runs_to_rle(case[0], starts.cpu().numpy(), ends.cpu().numpy(), bounds.cpu().numpy()) == brute_union(case)


# ---- stitch_results ---------------------------------------------------------------------------------------------------
def masks_of(out):
    return [(i['label_id'], i['conf'], i['pred_mask']) for i in out['pred_instances']]


@pytest.mark.parametrize('case', E2E_CASES + [(1, 30000, 2.0, 0.5, True)])
def test_stitch_results_device_equals_numpy(case):
    data = e2e_case(*case)
    xyz, inst, sem, tiles, results = data
    kw = dict(coords=xyz, gt=dict(semantic_labels=sem))
    out = stitch_results(results, tiles, backend='device', **kw)
    check_e2e(out, data, thinned=len(case) == 5)
    ref = stitch_results(results, tiles, backend='numpy', **kw)
    assert masks_of(out) == masks_of(ref)
    assert masks_of(stitch_results(results, tiles, backend='device', **kw)) == masks_of(out)
    for measure, thr in (('min', 0.9), ('iou', 0.999)):
        a = stitch_results(results, tiles, thr=thr, measure=measure, drop_margin_only=False, backend='device')
        b = stitch_results(results, tiles, thr=thr, measure=measure, drop_margin_only=False, backend='numpy')
        assert masks_of(a) == masks_of(b)


def test_stitch_results_device_keeps_cuda_arrays_on_the_device():
    xyz, inst, sem, tiles, results = e2e_case(*E2E_CASES[2])
    d_tiles = tile_cloud(dev(xyz), size=1.5, margin=0.3, origin=(-0.5, -0.5), backend='device')
    assert np.array_equal(d_tiles.tile_points.cpu().numpy(), tiles.tile_points)
    on_dev = [{k: (dev(v) if k in ('semantic_preds', 'offset_preds') else v) for k, v in r.items()} for r in results]
    out = stitch_results(on_dev, d_tiles, backend='device')
    ref = stitch_results(results, tiles, backend='numpy')
    assert out['semantic_preds'].is_cuda and out['offset_preds'].is_cuda
    assert np.array_equal(out['semantic_preds'].cpu().numpy(), ref['semantic_preds'])
    assert np.array_equal(out['offset_preds'].cpu().numpy(), ref['offset_preds'])
    assert masks_of(out) == masks_of(ref)


def test_drop_margin_only_device():
    tiles, res, margin_ids = margin_only_case()
    for drop in (True, False):
        a = stitch_results(res, tiles, drop_margin_only=drop, backend='device')
        b = stitch_results(res, tiles, drop_margin_only=drop, backend='numpy')
        assert masks_of(a) == masks_of(b) and len(a['pred_instances']) == (2 if drop else 4)


def test_stitch_results_beyond_the_device_range(monkeypatch):
    """16 385 real masks are far too many for a test: the range answer is replaced, the route is the real one"""
    from softgroup_amd.util import stitch as US
    xyz, inst, sem, tiles, results = e2e_case(*E2E_CASES[2])
    want = stitch_results(results, tiles, backend='numpy')
    monkeypatch.setattr(ST, 'stitch_supported', lambda n_inst, total, n_points: False)
    with pytest.raises(L.SoftGroupHipError):
        stitch_results(results, tiles, backend='device')
    monkeypatch.setattr(ST, '_AUTO', dict(ST._AUTO, stitch='device'))
    assert masks_of(stitch_results(results, tiles, backend='auto')) == masks_of(want)
    monkeypatch.setattr(ST, 'stitch_supported', lambda n_inst, total, n_points: total == 0)      # the populations decide
    assert masks_of(stitch_results(results, tiles, backend='auto')) == masks_of(want)
    monkeypatch.undo()
    assert not ST.stitch_supported(16385, 0, 1000) and ST.stitch_supported(16384, 2**31 - 1, 2**31 - 1)
    assert not ST.stitch_supported(10, 2**31, 1000) and not ST.stitch_supported(10, 10, 2**31)
    assert US._stitch_device is not None
    adj = torch.zeros((1, 1), dtype=torch.int32, device='cuda')
    with pytest.raises(L.SoftGroupHipError):
        ST.stitch_components(adj, 16385)


def test_tiled_scan_of_a_scene_stitched():
    """tile, scan every tile with the tiny model, stitch: structure only"""
    xyz, rgb, inst = synthetic.scene_s2(seed=1, n=30000, room_scale=0.45)      # (the density the grouping head needs)
    sem = np.where(inst >= 0, 2 + inst % 18, 0).astype(np.int64)
    tiles = tile_cloud(xyz, size=1.5, margin=0.2, origin=(-0.1, -0.1), backend='device')
    assert 2 <= len(tiles) <= 9
    model = synthetic.build_model(seed=0)
    results = []
    with torch.no_grad():
        for ids in tiles.point_ids:
            t_xyz, t_rgb, t_sem, t_inst = apply_sample(ids, xyz, rgb, sem, inst)
            results.append(model(synthetic.make_batch(t_xyz, t_rgb, instance_labels=t_inst, semantic_labels=t_sem)))
    full = stitch_results(results, tiles, coords=xyz, gt=dict(semantic_labels=sem, instance_labels=inst), backend='device')
    n = xyz.shape[0]
    core_tile, core_pos = np.asarray(tiles.core_tile), np.asarray(tiles.core_pos)
    for key in ('semantic_preds', 'offset_preds'):
        big = np.concatenate([np.asarray(r[key]) for r in results])
        assert np.array_equal(np.asarray(full[key]), big[np.asarray(tiles.offsets[:-1])[core_tile] + core_pos])
    assert 'panoptic_preds' not in full and full['instance_labels'] is inst
    flat = [i for r in results for i in r['pred_instances']]
    assert len(flat) > 0 and 0 < len(full['pred_instances']) <= len(flat)
    labels, confs = {i['label_id'] for i in flat}, {i['conf'] for i in flat}
    for g in full['pred_instances']:
        assert g['pred_mask']['length'] == n and g['label_id'] in labels and g['conf'] in confs
    ref = stitch_results(results, tiles, backend='numpy')
    assert masks_of(full) == masks_of(ref)
    assert rle_decode(full['pred_instances'][0]['pred_mask']).shape[0] == n
