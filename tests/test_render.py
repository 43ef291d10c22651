"""The render stage on the CPU: the numpy twins of ops/render.py against a plain per-pixel Python loop written from
the rules of include/softgroup_hip.h, the cameras, the PNG writer and reader, argument errors, the device-range rule,
and render_result / save_renders / tools/render.py on the numpy backend."""
import math
import os
import struct
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import render_cases as rc  # noqa: E402
from softgroup_amd.ops import render as RO  # noqa: E402
from softgroup_amd.util import render as UR  # noqa: E402
from softgroup_amd.util import visualize as V  # noqa: E402
from softgroup_amd.util import save_results  # noqa: E402
from softgroup_amd.util.rle import rle_encode  # noqa: E402

F64, F32 = np.float64, np.float32
ALL_ONES = (1 << 64) - 1


def ord32(d):
    bits, = struct.unpack('<I', struct.pack('<f', d))
    return (~bits & 0xFFFFFFFF) if bits >> 31 else (bits | 0x80000000)


def ord32_decode(k):
    return struct.unpack('<f', struct.pack('<I', (k ^ 0x80000000) if k >> 31 else (~k & 0xFFFFFFFF)))[0]


def brute_rasterize(coords, cams, width, height, point_size, world_radius):
    """the rules, one point and one pixel at a time, in numpy float64 scalars (IEEE, one rounding per operation)"""
    n_views = len(cams)
    keys = [[ALL_ONES] * (width * height) for _ in range(n_views)]
    culled = [0] * n_views
    with np.errstate(all='ignore'):
        for v, c in enumerate(cams):
            c = [F64(t) for t in c]
            for i, p in enumerate(coords):
                dx, dy, dz = F64(p[0]) - c[1], F64(p[1]) - c[2], F64(p[2]) - c[3]
                xc = (c[4] * dx + c[5] * dy) + c[6] * dz
                yc = (c[7] * dx + c[8] * dy) + c[9] * dz
                zc = (c[10] * dx + c[11] * dy) + c[12] * dz
                vis = True
                if c[16] != 0:
                    vis = bool(zc >= c[17])
                if c[18] != 0:
                    vis = vis and bool(zc <= c[19])
                if c[0] != 0:
                    pu, pv = c[14] + c[13] * xc, c[15] - c[13] * yc
                else:
                    pu, pv = c[14] + c[13] * (xc / zc), c[15] - c[13] * (yc / zc)
                if not (vis and -2.0**30 < pu < 2.0**30 and -2.0**30 < pv < 2.0**30):
                    culled[v] += 1
                    continue
                px, py = math.floor(pu), math.floor(pv)
                r = point_size
                if world_radius is not None:
                    rd = np.floor(c[13] * F64(world_radius)) if c[0] != 0 else np.floor(c[13] * (F64(world_radius) / zc))
                    r = min(16, int(rd)) if rd < 1e9 else 16
                    assert r >= 0
                d = F32(zc) + F32(0.0)
                key = (ord32(float(d)) << 32) | i
                for b in range(-r, r + 1):
                    for a in range(-r, r + 1):
                        x, y = px + a, py + b
                        if 0 <= x < width and 0 <= y < height and key < keys[v][y * width + x]:
                            keys[v][y * width + x] = key
    index = np.array([[-1 if k == ALL_ONES else k & 0xFFFFFFFF for k in row] for row in keys], np.int64)
    depth = np.array([[math.inf if k == ALL_ONES else ord32_decode(k >> 32) for k in row] for row in keys], F32)
    shape = (n_views, height, width)
    return index.astype(np.int32).reshape(shape), depth.reshape(shape), np.array(culled, np.int32)


def brute_shade(index, depth, colors, background, edl):
    n_views, height, width = index.shape
    image = np.zeros((n_views, height, width, 3), np.uint8)
    for v in range(n_views):
        for y in range(height):
            for x in range(width):
                i = int(index[v, y, x])
                if i < 0:
                    image[v, y, x] = background
                    continue
                c = [int(t) for t in colors[i]]
                if edl is not None:
                    strength, s, scale = edl
                    total, count = 0.0, 0
                    for ox, oy in ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1)):
                        nx, ny = x + ox * s, y + oy * s
                        if not (0 <= nx < width and 0 <= ny < height):
                            continue
                        count += 1
                        if index[v, ny, nx] < 0:
                            continue
                        t = float(depth[v, y, x]) - float(depth[v, ny, nx])
                        t = t if t > 0.0 else 0.0
                        t = t / scale
                        t = t if t < 1.0 else 1.0
                        total = total + t
                    resp = total / float(count) if count else 0.0
                    shade = 1.0 / (1.0 + strength * resp)
                    c = [math.floor(float(t) * shade + 0.5) for t in c]
                image[v, y, x] = c
    return image


_TWIN = {}


def twin(name):
    if name not in _TWIN:
        _TWIN[name] = RO.rasterize_numpy(*rc.raster_args(rc.RASTER[name]))
    return _TWIN[name]


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the twins against the loop ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(rc.RASTER))
def test_rasterize_numpy_equals_the_plain_loop(name):
    c = rc.RASTER[name]
    index, depth, culled = twin(name)
    want = brute_rasterize(*rc.raster_args(c))
    assert same(index, want[0]) and same(depth, want[1]) and same(culled, want[2])
    assert index.shape == (len(c['cams']), c['height'], c['width'])
    assert ((index < 0) == np.isposinf(depth)).all()


def test_the_cases_reach_what_they_were_built_for():
    index, depth, culled = twin('ties_equal')
    assert index[0, 3, 4] == 0 and index[0, 1, 1] == 64
    index, _, _ = twin('ties_round')
    assert [index[0, 2, k + 1] for k in range(3)] == [0, 2, 4]               # equal after rounding: the lower index
    index, _, _ = twin('ties_ulp')
    assert [index[0, 2, k + 1] for k in range(3)] == [1, 2, 5]               # one ulp nearer wins
    index, _, culled = twin('cull_near_far')
    assert culled.tolist() == [2] and set(index[index >= 0].tolist()) == {1, 2, 3, 4}
    _, _, culled = twin('cull_not_finite')
    assert culled.tolist() == [11, 12, 12]      # (1e30, 1e30, 1e30) projects to a finite u under the perspective
    index, _, culled = twin('cull_overflow')
    assert culled.tolist() == [3] and index[0, 4, 4] == 1      # two at inf, one finite beyond the window
    index, depth, _ = twin('ortho_negative')
    assert index[0, 2, 5] == 3 and index[0, 2, 7] == 5 and index[0, 2, 1] == 1
    assert not np.signbit(depth[0, 2, 5]) and not np.signbit(depth[0, 2, 7]) and depth[0, 4, 9] < 0
    index, _, _ = twin('world_radius_perspective')
    sizes = {i: int((index == i).sum()) for i in range(8)}
    assert sizes[0] == 1 and max(sizes.values()) > 17 * 17                    # r = 0 and a clipped r = 16
    for r in (0, 5, 16):
        index, _, _ = twin(f'world_radius_orthographic_{r}')
        cols = np.flatnonzero((index[0] >= 0).any(0))
        assert cols.size and (index[0] == 0).any(1).sum() <= 2 * r + 1
    # clipped on every side and on two sides at once
    index, _, _ = twin('scatter_257_33x17_ps2')
    assert all((index[0][s] >= 0).any() for s in ((0, slice(None)), (-1, slice(None)), (slice(None), 0), (slice(None), -1)))
    assert all(index[0][y, x] >= 0 for y in (0, -1) for x in (0, -1))
    c = rc.RASTER['lattice']
    u = c['cams'][0, 14] + c['cams'][0, 13] * c['coords'][:, 0].astype(F64)
    assert (u == np.floor(u)).sum() > 50 and (u != np.floor(u)).sum() > 50   # on the boundary, and a hair off it


def test_three_views_equal_three_single_calls():
    c = rc.RASTER['three_views']
    index, depth, culled = twin('three_views')
    for v in range(3):
        one = RO.rasterize_numpy(c['coords'], c['cams'][v:v + 1], c['width'], c['height'], c['point_size'])
        assert same(one[0], index[v:v + 1]) and same(one[1], depth[v:v + 1]) and same(one[2], culled[v:v + 1])


@pytest.mark.parametrize('case', rc.SHADE_CASES, ids=rc.SHADE_IDS)
def test_shade_numpy_equals_the_plain_loop(case):
    name, edl, background = case
    index, depth, _ = twin(name)
    colors = rc.colors_of(rc.RASTER[name])
    image = RO.shade_numpy(index, depth, colors, background, edl)
    assert same(image, brute_shade(index, depth, colors, background, edl))
    if edl is None or edl[0] == 0.0:
        flat = RO.shade_numpy(index, None, colors, background)
        assert same(image, flat)                                               # strength 0: colours unchanged
    elif name.startswith('scatter'):
        assert not same(image, RO.shade_numpy(index, None, colors, background))


def test_a_short_colour_array_raises():
    index, depth, _ = twin('scatter_1025_130x67_ps2')
    colors = rc.colors_of(rc.RASTER['scatter_1025_130x67_ps2'])
    with pytest.raises(ValueError, match='outside the'):
        RO.shade_numpy(index, depth, colors[:int(index.max())])
    RO.shade_numpy(index, depth, colors[:int(index.max()) + 1])


# ---- cameras -------------------------------------------------------------------------------------------------------
def test_look_at_is_orthonormal_and_right_handed():
    rng = np.random.default_rng(5)
    for _ in range(50):
        eye, target = rng.normal(size=3) * 10, rng.normal(size=3) * 10
        rot = UR.look_at(eye, target, rng.normal(size=3))
        assert np.allclose(rot @ rot.T, np.eye(3), atol=1e-12)
        assert np.allclose(np.cross(rot[0], rot[1]), -rot[2], atol=1e-12)      # right x up = -forward
        assert np.allclose(rot[2], (target - eye) / np.linalg.norm(target - eye))
    with pytest.raises(ValueError, match='parallel'):
        UR.look_at((0, 0, 5), (0, 0, 0))
    with pytest.raises(ValueError, match='different'):
        UR.look_at((1, 2, 3), (1, 2, 3))
    rot = UR.look_at((0, -5, 0), (0, 0, 0))                                    # from the front: x right, z up
    assert np.allclose(rot, [[1, 0, 0], [0, 0, 1], [0, 1, 0]])


@pytest.mark.parametrize('kind', ['perspective', 'orthographic'])
def test_fit_view_puts_the_whole_box_inside_the_image(kind):
    rng = np.random.default_rng(8)
    views = list(UR.VIEWS) + UR.turntable(5)
    for trial in range(12):
        lo = rng.normal(size=3) * 20
        hi = lo + rng.uniform(0.01, 30, 3) * rng.choice([1.0, 0.05], 3)
        width, height = [(64, 48), (48, 64), (33, 17), (200, 30), (1, 1), (2, 3)][trial % 6]
        corners = np.array([[(lo, hi)[a][0], (lo, hi)[b][1], (lo, hi)[c][2]] for a in (0, 1) for b in (0, 1)
                            for c in (0, 1)])
        pts = np.concatenate([corners, rng.uniform(lo, hi, (40, 3))]).astype(F32)
        lo32, hi32 = UR.cloud_bounds(pts)
        cams = [UR.named_view(v, lo32, hi32, (width, height), kind=kind, margin=(0.0, 0.05, 0.2)[trial % 3])
                for v in views]
        index, _, culled = RO.rasterize_numpy(pts, cams, width, height, 0)
        assert culled.tolist() == [0] * len(views)
        # every point landed inside: one that did not would own no pixel although nothing hides it from every side
        table = RO.camera_table(cams)
        for c in table:
            d = pts.astype(F64) - c[1:4]
            xc, yc, zc = d @ c[4:7], d @ c[7:10], d @ c[10:13]
            s = 1.0 if c[0] else 1.0 / zc
            u, v = c[14] + c[13] * xc * s, c[15] - c[13] * yc * s
            assert (u >= 0).all() and (u < width).all() and (v >= 0).all() and (v < height).all()
    with pytest.raises(ValueError, match='no finite point'):
        UR.cloud_bounds(np.full((3, 3), np.nan, F32))
    lo, hi = UR.cloud_bounds(np.array([[0, 0, 0], [np.nan, 9, 9], [1, 2, np.inf], [1, 1, 1]], F32))
    assert lo.tolist() == [0, 0, 0] and hi.tolist() == [1, 1, 1]


# ---- PNG -----------------------------------------------------------------------------------------------------------
def decode_png(data):
    """a decoder of its own: signature, chunks with their checksums, inflate, filter byte 0 per row"""
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    at, chunks = 8, []
    while at < len(data):
        length, kind = struct.unpack('>I4s', data[at:at + 8])
        body = data[at + 8:at + 8 + length]
        assert struct.unpack('>I', data[at + 8 + length:at + 12 + length])[0] == zlib.crc32(kind + body)
        chunks.append((kind, body))
        at += 12 + length
    assert [k for k, _ in chunks][0] == b'IHDR' and chunks[-1] == (b'IEND', b'')
    width, height, depth, colour, comp, filt, lace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(b''.join(b for k, b in chunks if k == b'IDAT'))
    rows = np.frombuffer(raw, np.uint8).reshape(height, 1 + 3 * width)
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(height, width, 3)


def test_png_round_trip_and_rejects(tmp_path):
    rng = np.random.default_rng(2)
    for k, shape in enumerate([(1, 1), (7, 5), (48, 131)]):
        image = rng.integers(0, 256, shape + (3,)).astype(np.uint8)
        path = str(tmp_path / f'{k}.png')
        size = UR.write_png(path, image)
        data = open(path, 'rb').read()
        assert size == len(data)
        assert same(UR.read_png(path), image) and same(np.ascontiguousarray(decode_png(data)), image)
    # a palette file: colour type 3 with a PLTE chunk
    rows = b''.join(b'\x00' + bytes([0, 1, 0, 1]) for _ in range(2))
    palette = UR._PNG_MAGIC + UR._chunk(b'IHDR', struct.pack('>IIBBBBB', 4, 2, 8, 3, 0, 0, 0)) + \
        UR._chunk(b'PLTE', bytes([0, 0, 0, 255, 255, 255])) + UR._chunk(b'IDAT', zlib.compress(rows)) + \
        UR._chunk(b'IEND', b'')
    (tmp_path / 'palette.png').write_bytes(palette)
    with pytest.raises(ValueError):
        UR.read_png(str(tmp_path / 'palette.png'))
    grey = UR._PNG_MAGIC + UR._chunk(b'IHDR', struct.pack('>IIBBBBB', 4, 2, 8, 0, 0, 0, 0)) + \
        UR._chunk(b'IDAT', zlib.compress(rows)) + UR._chunk(b'IEND', b'')
    (tmp_path / 'grey.png').write_bytes(grey)
    with pytest.raises(ValueError, match='8-bit RGB'):
        UR.read_png(str(tmp_path / 'grey.png'))
    filtered = UR._PNG_MAGIC + UR._chunk(b'IHDR', struct.pack('>IIBBBBB', 1, 1, 8, 2, 0, 0, 0)) + \
        UR._chunk(b'IDAT', zlib.compress(b'\x01\x05\x06\x07')) + UR._chunk(b'IEND', b'')
    (tmp_path / 'filtered.png').write_bytes(filtered)
    with pytest.raises(ValueError, match='filter'):
        UR.read_png(str(tmp_path / 'filtered.png'))
    broken = bytearray(open(str(tmp_path / '1.png'), 'rb').read())
    broken[40] ^= 1
    (tmp_path / 'broken.png').write_bytes(bytes(broken))
    with pytest.raises(ValueError, match='broken'):
        UR.read_png(str(tmp_path / 'broken.png'))
    with pytest.raises(ValueError):
        UR.write_png(str(tmp_path / 'x.png'), np.zeros((4, 4), np.uint8))


def test_montage():
    images = np.arange(5 * 2 * 3 * 3, dtype=np.uint8).reshape(5, 2, 3, 3)
    sheet = UR.montage(images, 2, background=(9, 8, 7))
    assert sheet.shape == (6, 6, 3)
    assert same(sheet[2:4, 3:6], images[3]) and same(sheet[4:6, 0:3], images[4])
    assert (sheet[4:6, 3:6] == (9, 8, 7)).all()
    assert same(UR.montage(list(images[:3]), 8), np.concatenate(list(images[:3]), axis=1))


# ---- arguments and the device range --------------------------------------------------------------------------------
def test_argument_errors():
    c = rc.RASTER['three_views']
    good = rc.raster_args(c)
    for bad in (dict(point_size=17), dict(point_size=-1), dict(point_size=1.5), dict(point_size=True),
                dict(world_radius=0.0), dict(world_radius=-1.0), dict(world_radius=np.nan)):
        kw = dict(point_size=good[4], world_radius=good[5])
        kw.update(bad)
        with pytest.raises(ValueError):
            RO.rasterize_numpy(good[0], good[1], good[2], good[3], **kw)
    with pytest.raises(ValueError):
        RO.rasterize_numpy(good[0], good[1], 0, 5)
    with pytest.raises(ValueError):
        RO.rasterize_numpy(good[0][:, :2], good[1], 5, 5)
    with pytest.raises(ValueError, match='near > 0'):
        RO.camera_table(rc.Camera('perspective', (0, 0, 0), np.eye(3), 1.0, 0.5, 0.5, None, None))
    with pytest.raises(ValueError, match='near > 0'):
        RO.camera_table(rc.Camera('perspective', (0, 0, 0), np.eye(3), 1.0, 0.5, 0.5, 0.0, None))
    with pytest.raises(ValueError, match='f > 0'):
        RO.camera_table(rc.Camera('orthographic', (0, 0, 0), np.eye(3), 0.0, 0.5, 0.5, None, None))
    with pytest.raises(ValueError, match='finite'):
        RO.camera_table(rc.Camera('orthographic', (0, np.nan, 0), np.eye(3), 1.0, 0.5, 0.5, None, None))
    with pytest.raises(ValueError, match='kind'):
        RO.camera_table(rc.Camera('fisheye', (0, 0, 0), np.eye(3), 1.0, 0.5, 0.5, None, None))
    with pytest.raises(ValueError):
        RO.camera_table([])
    index, depth, _ = twin('three_views')
    colors = rc.colors_of(c)
    for edl in ((-1.0, 1, 1.0), (1.0, 0, 1.0), (1.0, 5, 1.0), (1.0, 1, 0.0), (1.0, 1.5, 1.0)):
        with pytest.raises(ValueError):
            RO.shade_numpy(index, depth, colors, edl=edl)
    with pytest.raises(ValueError):
        RO.shade_numpy(index, depth, colors, background=(0, 0, 256))
    with pytest.raises(ValueError):
        RO.shade_numpy(index, depth, colors.astype(np.int32))
    with pytest.raises(ValueError):
        RO.rasterize(good[0], good[1], good[2], good[3], backend='cuda')


def test_device_range_rule(monkeypatch):
    assert RO.in_device_range(0, 1, 1, 1) and RO.in_device_range(2**31 - 2, 16, 2048, 2048)
    assert RO.in_device_range(5, 1, 8192, 8192)
    for n, v, w, h in ((2**31 - 1, 1, 8, 8), (5, 17, 8, 8), (5, 0, 8, 8), (5, 1, 8193, 8), (5, 1, 8, 8193),
                       (5, 2, 8192, 8192), (5, 16, 2048, 2049)):
        assert not RO.in_device_range(n, v, w, h)
    assert (RO.MAX_RADIUS, RO.MAX_VIEWS, RO.MAX_SIDE, RO.MAX_PIXELS) == (16, 16, 8192, 2**26)
    assert set(RO._AUTO) == {'rasterize', 'shade'} and set(RO._AUTO.values()) <= {'device', 'numpy'}
    # beyond the range 'auto' takes numpy even where the table says device; 'device' raises and launches nothing
    import torch
    from softgroup_amd import _lib
    monkeypatch.setattr(RO, '_AUTO', {'rasterize': 'device', 'shade': 'device'})
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(_lib, 'lib', lambda: pytest.fail('nothing may be launched'))
    c = rc.RASTER['one_pixel']
    cams17 = np.repeat(c['cams'], 17, axis=0)
    out = RO.rasterize(c['coords'], cams17, 1, 1, 0, backend='auto')
    assert out[0].shape == (17, 1, 1) and (out[0] == 0).all()
    with pytest.raises(_lib.SoftGroupHipError, match='outside the supported range'):
        RO.rasterize(c['coords'], cams17, 1, 1, 0, backend='device')
    image = RO.shade(out[0], out[1], rc.colors_of(c), backend='auto')
    assert image.shape == (17, 1, 1, 3)
    with pytest.raises(_lib.SoftGroupHipError, match='outside the supported range'):
        RO.shade(out[0], out[1], rc.colors_of(c), backend='device')


# ---- results, trees and the command line -----------------------------------------------------------------------------
def synthetic_result(seed=4, n=400):
    rng = np.random.default_rng(seed)
    coords = (rng.uniform(-1, 1, (n, 3)) * (3, 2, 1)).astype(F32)
    inst = (coords[:, 0] > 0).astype(np.int64) + 2 * (coords[:, 1] > 0)
    sem = inst % 3
    sem_label = sem.copy()
    sem_label[:7] = -100
    masks = [(inst == k) & (rng.random(n) < 0.9) for k in range(4)]
    return dict(scan_id='scene_r', coords_float=coords, color_feats=rng.uniform(-1, 1, (n, 3)).astype(F32),
                semantic_labels=sem_label, semantic_preds=(sem + (rng.random(n) < 0.1)) % 3,
                offset_preds=(rng.normal(size=(n, 3)) * 0.05).astype(F32), offset_labels=np.zeros((n, 3), F32),
                gt_instances=np.where(sem_label >= 0, (sem + 1) * 1000 + inst + 1, 0).astype(np.int64),
                pred_instances=[dict(scan_id='scene_r', label_id=int(k % 3) + 1, conf=0.2 + 0.15 * k,
                                     pred_mask=rle_encode(m.astype(np.int64))) for k, m in enumerate(masks)])


class Dataset:
    NYU_ID = None


@pytest.mark.parametrize('task', V.TASKS)
def test_render_result_every_task(task):
    result = synthetic_result()
    image, index, depth = UR.render_result(result, task, views=('iso', 'top'), size=(48, 36), backend='numpy',
                                           return_buffers=True)
    assert image.shape == (2, 36, 48, 3) and image.dtype == np.uint8
    xyz, rgb = V.colors_from_result(result, task, backend='numpy')
    assert len(xyz) == 393 and index.max() < 393 and (index >= 0).sum() > 300
    colors = UR._as_uint8(rgb)
    owned = index >= 0
    assert same(image[owned], colors[index[owned]]) and (image[~owned] == 255).all()
    lit = UR.render_result(result, task, views=('iso', 'top'), size=(48, 36), backend='numpy', edl=True,
                           background=(0, 0, 0))
    assert (lit[~owned] == 0).all() and (lit[owned] <= image[owned]).all() and (lit[owned] < image[owned]).any()


def test_save_renders_and_the_command_line(tmp_path):
    result = synthetic_result()
    root = str(tmp_path / 'results')
    save_results(root, [result], ['semantic', 'instance'], Dataset, backend='numpy')
    out = str(tmp_path / 'png')
    infos = UR.save_renders(root, ['scene_r'], V.TASKS, out, views=('iso', 'front'), size=(40, 30), backend='numpy')
    assert [os.path.basename(i['path']) for i in infos] == [f'scene_r_{t}.png' for t in V.TASKS]
    # one rasterisation for the tasks that share the input coordinates, one for the shifted cloud
    assert [i['rasterized'] for i in infos] == [t in ('input', 'offset_semantic_pred') for t in V.TASKS]
    for info in infos:
        sheet = UR.read_png(info['path'])
        assert sheet.shape == (30, 80, 3) and info['size'] == (80, 30) and info['views'] == 2
        want = UR.render_result(result, info['task'], views=('iso', 'front'), size=(40, 30), backend='numpy')
        assert same(sheet, UR.montage(want, 2)), info['task']
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tools'))
    import importlib
    tool = importlib.import_module('render')
    one = str(tmp_path / 'one.png')
    assert tool.main(['--prediction_path', root, '--room_name', 'scene_r', '--task', 'semantic_pred', '--views', 'iso',
                      'front', '--size', '40', '30', '--backend', 'numpy', '--out', one]) == 0
    assert same(UR.read_png(one), UR.read_png(os.path.join(out, 'scene_r_semantic_pred.png')))
    assert sorted(os.listdir(str(tmp_path))) == ['one.png', 'png', 'results']
    assert tool.main(['--prediction_path', root, '--all-rooms', '--task', 'input', 'instance_gt', '--size', '20', '10',
                      '--edl', '--world-radius', '0.05', '--backend', 'numpy', '--out-dir', str(tmp_path / 'all')]) == 0
    assert sorted(os.listdir(str(tmp_path / 'all'))) == ['scene_r_input.png', 'scene_r_instance_gt.png']
    np.savetxt(str(tmp_path / 'cloud.txt'), np.concatenate([result['coords_float'],
                                                            np.full((400, 3), 200.0)], axis=1), fmt='%.6f')
    assert tool.main(['--cloud', str(tmp_path / 'cloud.txt'), '--views', 'top', '--size', '16', '12', '--orthographic',
                      '--backend', 'numpy', '--out', str(tmp_path / 'cloud.png')]) == 0
    picture = UR.read_png(str(tmp_path / 'cloud.png'))
    assert picture.shape == (12, 16, 3) and (picture == 200).all(2).any() and (picture == 255).all(2).any()
    with pytest.raises(SystemExit):
        tool.main(['--prediction_path', root, '--all-rooms'])
    with pytest.raises(SystemExit):
        tool.main(['--prediction_path', root, '--room_name', 'scene_r', '--out', str(tmp_path / 'a.jpg')])
