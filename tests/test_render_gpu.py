"""The render kernels of csrc/render.hip against the numpy twins of ops/render.py, byte for byte, on the shared case
list of render_cases.py, one cloud above the launch cap of the splat kernel, and the calls of util/render.py on both
backends."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import render_cases as rc  # noqa: E402
from softgroup_amd.ops import render as RO  # noqa: E402
from softgroup_amd.util import render as UR  # noqa: E402
from softgroup_amd.util import visualize as V  # noqa: E402

pytestmark = pytest.mark.gpu

# one trip of the splat kernel's stride loop covers kRenderMaxBlocks * kRenderBlock points (tests/test_render_caps.py
# pins both numbers to the source): the cloud below needs a second trip, and its last wave is partial
SPLAT_CAP = 2048 * 256
ABOVE_CAP_POINTS = SPLAT_CAP + 16 * 64 + 5

_TWIN = {}


def twin(name):
    if name not in _TWIN:
        _TWIN[name] = RO.rasterize_numpy(*rc.raster_args(rc.RASTER[name]))
    return _TWIN[name]


def same(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def on_device(c):
    return torch.from_numpy(c['coords']).cuda()


@pytest.mark.parametrize('name', sorted(rc.RASTER))
def test_rasterize_equals_the_twin(name):
    c = rc.RASTER[name]
    args = rc.raster_args(c)
    got = RO.rasterize(on_device(c), *args[1:], backend='device')
    assert all(t.is_cuda for t in got)
    for g, w, what in zip(got, twin(name), ('index', 'depth', 'culled')):
        assert same(g, w), what
    again = RO.rasterize(on_device(c), *args[1:], backend='device')
    assert all(same(a, g.cpu().numpy()) for a, g in zip(again, got))          # two calls, the same bytes
    host = RO.rasterize(*args, backend='device')                              # numpy in, numpy out
    assert all(isinstance(h, np.ndarray) and same(h, w) for h, w in zip(host, twin(name)))
    cpu = RO.rasterize(torch.from_numpy(c['coords']), *args[1:], backend='device')     # a CPU tensor: as numpy
    assert all(isinstance(h, np.ndarray) and same(h, w) for h, w in zip(cpu, twin(name)))


@pytest.mark.parametrize('case', rc.SHADE_CASES, ids=rc.SHADE_IDS)
def test_shade_equals_the_twin(case):
    name, edl, background = case
    index, depth, _ = twin(name)
    colors = rc.colors_of(rc.RASTER[name])
    want = RO.shade_numpy(index, depth, colors, background, edl)
    d_index, d_depth, d_colors = (torch.from_numpy(a).cuda() for a in (index, depth, colors))
    got = RO.shade(d_index, d_depth, d_colors, background, edl, backend='device')
    assert got.is_cuda and same(got, want)
    assert same(RO.shade(d_index, d_depth, d_colors, background, edl, backend='device'), want)
    assert same(RO.shade(index, depth, colors, background, edl, backend='device'), want)


def test_a_short_colour_array_raises_and_is_never_read():
    index, depth, _ = twin('scatter_1025_130x67_ps2')
    colors = rc.colors_of(rc.RASTER['scatter_1025_130x67_ps2'])
    d_index, d_depth = torch.from_numpy(index).cuda(), torch.from_numpy(depth).cuda()
    for edl in (None, (1.0, 1, 0.3)):
        with pytest.raises(ValueError, match='outside the'):
            RO.shade(d_index, d_depth, torch.from_numpy(colors[:int(index.max())]).cuda(), edl=edl, backend='device')
        with pytest.raises(ValueError, match='outside the'):
            RO.shade(d_index, d_depth, torch.zeros((0, 3), dtype=torch.uint8).cuda(), edl=edl, backend='device')
    short = torch.from_numpy(colors[:int(index.max()) + 1]).cuda()
    assert same(RO.shade(d_index, d_depth, short, backend='device'), RO.shade_numpy(index, depth, colors))


def test_above_the_launch_cap():
    """point_size 0 into a 64 x 48 image: every pixel is fought over by ~150 points of the first trip of the stride
    loop, and the points of the second trip lie in front of them"""
    rng = np.random.default_rng(17)
    cam = rc.persp(64, 48)
    z = rng.uniform(1.0, 3.0, ABOVE_CAP_POINTS)
    z[SPLAT_CAP:] = rng.uniform(0.8, 0.9, ABOVE_CAP_POINTS - SPLAT_CAP)
    u, v = rng.uniform(-2, 66, z.size), rng.uniform(-2, 50, z.size)
    pts = np.stack([(u - cam.cx) * z / cam.f, -(v - cam.cy) * z / cam.f, z], 1).astype(np.float32)
    pts[-3:] = [[0.0, 0.0, 0.75], [np.nan, 0.0, 1.0], [0.01, 0.01, 0.25]]     # the last (partial) wave: a winner, two culled
    want = RO.rasterize_numpy(pts, cam, 64, 48, 0)
    assert want[0][0, 24, 32] == ABOVE_CAP_POINTS - 3 and want[2].tolist() == [2]
    assert (want[0] >= SPLAT_CAP).sum() > 500 and (want[0] >= 0).all()
    got = RO.rasterize(torch.from_numpy(pts).cuda(), cam, 64, 48, 0, backend='device')
    assert all(same(g, w) for g, w in zip(got, want))


def test_cuda_in_gives_cuda_out_without_a_host_copy_of_the_cloud(monkeypatch):
    rng = np.random.default_rng(23)
    xyz = (rng.uniform(-1, 1, (5000, 3)) * (3, 2, 1)).astype(np.float32)
    xyz[7] = np.nan                                                           # (left out of the box, culled)
    rgb = rng.integers(0, 256, (5000, 3)).astype(np.uint8)
    kw = dict(views=('iso', 'top', 'front', 'side'), size=(96, 64), point_size=1, edl=True, return_buffers=True)
    want = UR.render_cloud(xyz, rgb, backend='numpy', **kw)
    d_xyz, d_rgb = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda()
    to_cpu, to_numpy = torch.Tensor.cpu, torch.Tensor.numpy

    def small(fn):
        def guarded(t, *a, **k):
            assert t.numel() <= 64, 'a large tensor went to the host'       # (the box of the cloud is 6 numbers)
            return fn(t, *a, **k)
        return guarded

    monkeypatch.setattr(torch.Tensor, 'cpu', small(to_cpu))
    monkeypatch.setattr(torch.Tensor, 'numpy', small(to_numpy))
    got = UR.render_cloud(d_xyz, d_rgb, backend='device', **kw)
    monkeypatch.undo()
    assert all(g.is_cuda for g in got) and all(same(g, w) for g, w in zip(got, want))
    # numpy in, numpy out on the device backend; a CUDA cloud on the numpy backend still gives CUDA out
    host = UR.render_cloud(xyz, rgb, backend='device', **kw)
    assert all(isinstance(h, np.ndarray) and same(h, w) for h, w in zip(host, want))
    back = UR.render_cloud(d_xyz, d_rgb, backend='numpy', **kw)
    assert all(b.is_cuda and same(b, w) for b, w in zip(back, want))


def test_device_range_raises_before_any_launch():
    from softgroup_amd import _lib
    c = rc.RASTER['one_pixel']
    cams17 = np.repeat(c['cams'], 17, axis=0)
    with pytest.raises(_lib.SoftGroupHipError, match='outside the supported range'):
        RO.rasterize(on_device(c), cams17, 1, 1, 0, backend='device')
    lib = _lib.lib()
    assert lib.sg_render_rasterize(None, 0, None, 17, 1, 1, 0, 0.0, 7, None, None, None, None, 0, None) != 0
    assert b'outside the supported range' in lib.sg_last_error()
    assert lib.sg_render_shade(None, None, 1, 8193, 1, None, 0, 0, 0, 0, 0, 0.0, 1, 1.0, None, None, None) != 0
    assert b'outside the supported range' in lib.sg_last_error()


@pytest.mark.parametrize('task', V.TASKS)
def test_render_result_device_equals_numpy(task):
    from test_render import synthetic_result
    result = synthetic_result()
    kw = dict(views=('iso', 'side'), size=(64, 48), edl=True, world_radius=0.05, return_buffers=True)
    want = UR.render_result(result, task, backend='numpy', **kw)
    got = UR.render_result(result, task, backend='device', **kw)
    assert all(same(g, w) for g, w in zip(got, want))


def test_save_renders_writes_the_same_pixels_with_both_backends(tmp_path):
    from test_render import Dataset, synthetic_result
    from softgroup_amd.util import save_results
    root = str(tmp_path / 'results')
    save_results(root, [synthetic_result()], ['semantic', 'instance'], Dataset, backend='numpy')
    kw = dict(views=('iso', 'top'), size=(64, 48), point_size=2, edl=True)
    a = UR.save_renders(root, ['scene_r'], V.TASKS, str(tmp_path / 'numpy'), backend='numpy', **kw)
    b = UR.save_renders(root, ['scene_r'], V.TASKS, str(tmp_path / 'device'), backend='device', **kw)
    assert [i['rasterized'] for i in a] == [i['rasterized'] for i in b]
    for x, y in zip(a, b):
        assert os.path.basename(x['path']) == os.path.basename(y['path'])
        assert same(UR.read_png(x['path']), UR.read_png(y['path'])), x['task']
        assert open(x['path'], 'rb').read() == open(y['path'], 'rb').read()
