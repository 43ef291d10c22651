"""Keeps the sizes of tests/test_render_gpu.py honest: the launch cap of the splat kernel, its block size and the
largest splat radius are read out of csrc/render.hip, and the point count of the GPU test that is meant to make a
second trip through the stride loop must sit on the far side of the cap.  The Python limits of ops/render.py are held
to the same source."""
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import torch  # noqa: E402

_GPU_UP_BEFORE = torch.cuda.is_initialized()
import test_render_gpu as G  # noqa: E402

_GPU_UP_AFTER = torch.cuda.is_initialized()

PKG = os.path.join(os.path.dirname(HERE), 'softgroup_amd')
with open(os.path.join(PKG, 'csrc', 'render.hip')) as f:
    SRC = f.read()


def _const(name, ctype='int'):
    m = re.search(r'constexpr\s+' + ctype + r'\s+' + name + r'\s*=\s*([^;]+);', SRC)
    assert m, f'constexpr {ctype} {name} not found'
    return m.group(1).strip()


def test_importing_the_gpu_module_does_not_touch_the_gpu():
    assert _GPU_UP_BEFORE or not _GPU_UP_AFTER
    assert G.pytestmark.name == 'gpu'


def test_the_cloud_above_the_cap_is_above_the_cap():
    block, blocks = int(_const('kRenderBlock')), int(_const('kRenderMaxBlocks'))
    # the splat launch uses exactly these two, a lane per point
    assert re.search(r'render_splat_kernel<<<\s*grid_for\(\s*n\s*,\s*kRenderBlock\s*,\s*kRenderMaxBlocks\s*\)\s*,\s*'
                     r'kRenderBlock\s*,', SRC)
    assert re.search(r'base \+= stride', SRC) and re.search(r'stride = static_cast<int64_t>\(gridDim\.x\) \* kRenderBlock', SRC)
    cap = block * blocks
    assert cap == G.SPLAT_CAP
    assert cap < G.ABOVE_CAP_POINTS < 2 * cap                                  # a second trip
    assert G.ABOVE_CAP_POINTS % 64 and (G.ABOVE_CAP_POINTS - cap) > 64        # whole waves and a partial last one
    assert block % 64 == 0


def test_python_limits_equal_the_source():
    from softgroup_amd.ops import render as RO
    assert int(_const('kRenderMaxRadius')) == RO.MAX_RADIUS == 16
    assert int(_const('kRenderMaxViews')) == RO.MAX_VIEWS
    assert int(_const('kRenderMaxSide')) == RO.MAX_SIDE
    assert _const('kRenderMaxPixels', 'int64_t') == '1LL << 26' and RO.MAX_PIXELS == 1 << 26
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'softgroup_hip.h')).read()
    assert int(re.search(r'#define SG_RENDER_CAMERA_DOUBLES (\d+)', header).group(1)) == RO.CAMERA_DOUBLES
    assert int(re.search(r'#define SG_RENDER_FLAG_COLOR_INDEX (\d+)', header).group(1)) == RO.FLAG_COLOR_INDEX
    assert int(re.search(r'#define SG_RENDER_STAGE_ALL (\d+)', header).group(1)) == RO._STAGE_ALL
    # the radius loop of the kernel is bounded by the constant, whatever the arguments say
    assert re.search(r'r = r < 0 \? 0 : \(r > kRenderMaxRadius \? kRenderMaxRadius : r\);', SRC)
    # the order of the eight neighbours, kernel and twin
    dx = [int(v) for v in re.search(r'kEdlDx\[8\] = \{([^}]+)\}', SRC).group(1).split(',')]
    dy = [int(v) for v in re.search(r'kEdlDy\[8\] = \{([^}]+)\}', SRC).group(1).split(',')]
    assert tuple(zip(dx, dy)) == RO.EDL_NEIGHBOURS
