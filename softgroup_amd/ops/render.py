"""Result clouds to images (csrc/render.hip): ``rasterize``, a z-buffered point splat over several views at once, and
``shade``, the colour lookup with optional eye-dome lighting.

The reference has no counterpart (its docs send the user to a desktop viewer); the rules are this project's and are
stated in include/softgroup_hip.h:

cameras
  ``Camera(kind, eye, rot, f, cx, cy, near, far)``: ``kind`` 'perspective' or 'orthographic', ``rot`` the 3 x 3 rotation
  with rows (right, up, forward), ``near`` / ``far`` a number or None (a perspective camera needs ``near > 0``).
  ``camera_table`` packs them into the float64 rows [V, 20] BOTH backends read: the host computes every sine and
  cosine once, the device evaluates no transcendental function.
per (view, point i), every operation ONE IEEE double operation in this order
  ``dx = double(x) - ex`` (dy, dz likewise); ``xc = (r00 dx + r01 dy) + r02 dz``, yc and zc from rows 1 and 2;
  visible when ``zc >= near`` and ``zc <= far`` where given (a comparison with NaN is false: a coordinate that is not
  finite culls itself); perspective ``u = cx + f (xc / zc)``, ``v = cy - f (yc / zc)``, orthographic ``u = cx + f xc``,
  ``v = cy - f yc``; culled unless ``-2**30 < u < 2**30`` and the same for v, tested on the doubles; ``px = floor(u)``,
  ``py = floor(v)``; ``r = point_size`` or, with ``world_radius = w``, ``floor(f (w / zc))`` (perspective) or
  ``floor(f w)`` (orthographic) clipped to 0 .. 16; the point covers the pixels ``(px + a, py + b)``, a, b = -r .. r,
  inside the image (clipped per pixel); ``d = float32(zc) + 0.0f``; ``key = (ord32(d) << 32) | i``.  The owner of a
  pixel is the smallest key: the nearest depth after rounding to float32, the LOWEST index among equal depths.
outputs
  ``index`` int32 [V, H, W] (-1: empty), ``depth`` float32 [V, H, W] (+inf: empty), row 0 the top of the image, and
  ``culled`` int32 [V], the culled points of every view (not an error; on the device it stays there until read).
  Emptiness is ``index < 0``: a ``zc`` beyond the float32 range (an orthographic view without ``far`` whose eye lies
  ~3e38 from the cloud) rounds to ``d = +inf`` and the point still owns its pixel, with depth +inf, on both backends.
shading
  uint8 [V, H, W, 3]: the background for an empty pixel, ``colors[i]`` for a pixel of point i; an owner outside
  ``0 .. len(colors)-1`` raises ``ValueError`` (the device never dereferences it).  ``edl=(strength, radius, scale)``
  scales every channel: the eight neighbours ``EDL_NEIGHBOURS`` times the radius in that order, one outside the image
  not counted, an empty one 0, any other ``t = double(d) - double(dn)``, ``t = t if t > 0 else 0``, ``t = t / scale``,
  ``t = t if t < 1 else 1``; ``resp`` = the sum in that order / ``double(count)`` (0 without a counted neighbour);
  ``shade = 1 / (1 + strength resp)``; ``c' = uint8(floor(double(c) shade + 0.5))``.

Device range: ``0 <= N < 2**31 - 1``, 1 .. 16 views, sides 1 .. 8192, ``V H W <= 2**26``; beyond it ``'auto'`` takes
numpy and ``'device'`` raises, and nothing is launched.  CUDA in gives CUDA out, numpy in gives numpy out, under every
backend.  The ``*_numpy`` twins are the definition the device results are held to byte for byte.
"""
from collections import namedtuple

import numpy as np

from ._args import _host, _is_cuda, _upload, _xyz_numpy, choose_backend

__all__ = ['Camera', 'camera_table', 'auto_backend', 'in_device_range', 'rasterize', 'rasterize_numpy', 'shade',
           'shade_numpy', 'MAX_RADIUS', 'MAX_VIEWS', 'MAX_SIDE', 'MAX_PIXELS', 'MAX_DEVICE_POINTS', 'CAMERA_DOUBLES',
           'EDL_NEIGHBOURS', 'FLAG_COLOR_INDEX']

MAX_RADIUS = 16
MAX_VIEWS = 16
MAX_SIDE = 8192
MAX_PIXELS = 2**26
MAX_DEVICE_POINTS = 2**31 - 1
CAMERA_DOUBLES = 20
FLAG_COLOR_INDEX = 1
EDL_NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1))     # (dx, dy), dy > 0 is down
_WINDOW = np.float64(2**30)
_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
_STAGE_ALL = 7

# what backend='auto' means with a GPU present -- the single place to change.  An entry is 'device' only when the
# recorded table of tools/render_bench.py (profiles/render_bench.txt) shows the operation ahead on both clouds by more
# than the spread of the repetitions.  It does, for both: on numpy arrays in and out (upload and read-back included)
# ``rasterize`` and ``shade`` on the device are ahead of the twins in every row of the table, by one to two orders of
# magnitude, while the repetitions spread by a few per cent.
_AUTO = {'rasterize': 'device', 'shade': 'device'}

Camera = namedtuple('Camera', 'kind eye rot f cx cy near far')


def auto_backend(backend, what):
    """'device' or 'numpy' for one of the operations of ``_AUTO``"""
    return choose_backend(backend, _AUTO[what])


def camera_table(cameras):
    """a Camera or a sequence of them (or the table itself) -> float64 [V, 20], checked"""
    if isinstance(cameras, np.ndarray):
        table = np.ascontiguousarray(cameras, dtype=np.float64)
        if table.ndim != 2 or table.shape[1] != CAMERA_DOUBLES or table.shape[0] < 1:
            raise ValueError(f'cameras: a table [V, {CAMERA_DOUBLES}] with V >= 1')
    else:
        if isinstance(cameras, Camera):
            cameras = [cameras]
        cameras = list(cameras)
        if not cameras:
            raise ValueError('cameras: at least one view')
        table = np.zeros((len(cameras), CAMERA_DOUBLES), np.float64)
        for row, cam in zip(table, cameras):
            if cam.kind not in ('perspective', 'orthographic'):
                raise ValueError(f"camera kind {cam.kind!r}: 'perspective' or 'orthographic'")
            row[0] = float(cam.kind == 'orthographic')
            row[1:4] = np.asarray(cam.eye, np.float64).reshape(3)
            row[4:13] = np.asarray(cam.rot, np.float64).reshape(9)
            row[13], row[14], row[15] = cam.f, cam.cx, cam.cy
            if cam.near is not None:
                row[16], row[17] = 1.0, cam.near
            if cam.far is not None:
                row[18], row[19] = 1.0, cam.far
    if not np.isfinite(table).all():
        raise ValueError('cameras: every entry finite')
    if not (np.isin(table[:, 0], (0.0, 1.0)).all() and np.isin(table[:, [16, 18]], (0.0, 1.0)).all()):
        raise ValueError('cameras: kind and the near / far marks are 0 or 1')
    if not (table[:, 13] > 0).all():
        raise ValueError('cameras: f > 0')
    persp = table[:, 0] == 0.0
    if not ((table[persp, 16] == 1.0) & (table[persp, 17] > 0)).all():
        raise ValueError('cameras: a perspective camera needs near > 0')
    return table


def _size(width, height):
    for v in (width, height):
        if isinstance(v, bool) or int(v) != v or int(v) < 1:
            raise ValueError(f'image size {width!r} x {height!r}: integers >= 1')
    return int(width), int(height)


def _radius(point_size, world_radius):
    """-> (point_size, world_radius as a float, 0.0 without one)"""
    if world_radius is not None:
        w = float(world_radius)
        if not (w > 0 and np.isfinite(w)):
            raise ValueError(f'world_radius {world_radius!r}: None or a finite number > 0')
        return 0, w
    if isinstance(point_size, bool) or int(point_size) != point_size or not 0 <= int(point_size) <= MAX_RADIUS:
        raise ValueError(f'point_size {point_size!r}: an integer between 0 and {MAX_RADIUS}')
    return int(point_size), 0.0


def in_device_range(n, n_views, width, height):
    return (0 <= n < MAX_DEVICE_POINTS and 1 <= n_views <= MAX_VIEWS and 1 <= width <= MAX_SIDE
            and 1 <= height <= MAX_SIDE and n_views * width * height <= MAX_PIXELS)


def _edl(edl):
    if edl is None:
        return None
    if isinstance(edl, dict):
        edl = (edl['strength'], edl['radius'], edl['scale'])
    strength, radius, scale = edl
    if isinstance(radius, bool) or int(radius) != radius or not 1 <= int(radius) <= 4:
        raise ValueError(f'edl radius {radius!r}: an integer between 1 and 4 pixels')
    strength, scale = float(strength), float(scale)
    if not (strength >= 0 and np.isfinite(strength)) or not (scale > 0 and np.isfinite(scale)):
        raise ValueError('edl: strength >= 0 and scale > 0, both finite')
    return strength, int(radius), scale


def _background(background):
    bg = np.asarray(background).reshape(-1)
    if bg.size != 3 or bg.dtype.kind not in 'iu' or bg.min() < 0 or bg.max() > 255:
        raise ValueError('background: three integers 0 .. 255')
    return tuple(int(v) for v in bg)


# ---- the twins -------------------------------------------------------------------------------------------------------
def _ord32(d):
    bits = np.ascontiguousarray(d, np.float32).view(np.uint32)
    return np.where(bits >> np.uint32(31), ~bits, bits | np.uint32(0x80000000))


def _ord32_decode(k):
    k = np.ascontiguousarray(k, np.uint32)
    return np.where(k >> np.uint32(31), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def rasterize_numpy(coords, cameras, width, height, point_size=1, world_radius=None):
    """coords float32 [N, 3], cameras (``camera_table``) -> (index int32 [V, H, W], depth float32 [V, H, W], culled
    int32 [V]).  Elementwise float64 numpy in the order of the rules; ``np.minimum.at`` over the keys."""
    xyz = _xyz_numpy(coords, 'coords')
    cams = camera_table(cameras)
    width, height = _size(width, height)
    point_size, world = _radius(point_size, world_radius)
    n, n_views = xyz.shape[0], cams.shape[0]
    if n >= 2**32 - 1:
        raise ValueError('coords: fewer than 2**32 - 1 points (the key holds the point in 32 bits)')
    keys = np.full((n_views, height * width), _EMPTY, np.uint64)
    culled = np.zeros(n_views, np.int32)
    x, y, z = (xyz[:, k].astype(np.float64) for k in range(3))
    ids = np.arange(n, dtype=np.uint64)
    with np.errstate(all='ignore'):
        for v, c in enumerate(cams):
            ortho = c[0] != 0.0
            dx, dy, dz = x - c[1], y - c[2], z - c[3]
            xc = (c[4] * dx + c[5] * dy) + c[6] * dz
            yc = (c[7] * dx + c[8] * dy) + c[9] * dz
            zc = (c[10] * dx + c[11] * dy) + c[12] * dz
            f = c[13]
            vis = np.ones(n, bool)
            if c[16] != 0.0:
                vis = zc >= c[17]
            if c[18] != 0.0:
                vis = vis & (zc <= c[19])
            if ortho:
                pu, pv = c[14] + f * xc, c[15] - f * yc
            else:
                pu, pv = c[14] + f * (xc / zc), c[15] - f * (yc / zc)
            vis = vis & (pu > -_WINDOW) & (pu < _WINDOW) & (pv > -_WINDOW) & (pv < _WINDOW)
            culled[v] = n - int(vis.sum())
            if not vis.any():
                continue
            px, py = np.floor(pu[vis]).astype(np.int64), np.floor(pv[vis]).astype(np.int64)
            if world > 0.0:
                rd = np.full(px.shape, np.floor(f * world)) if ortho else np.floor(f * (world / zc[vis]))
                r = np.where(rd >= MAX_RADIUS, MAX_RADIUS, np.where(rd >= 0.0, rd, 0.0)).astype(np.int64)
            else:
                r = np.full(px.shape, point_size, np.int64)
            d = zc[vis].astype(np.float32) + np.float32(0.0)
            key = (_ord32(d).astype(np.uint64) << np.uint64(32)) | ids[vis]
            for b in range(-int(r.max()), int(r.max()) + 1):
                yy = py + b
                row_ok = (abs(b) <= r) & (yy >= 0) & (yy < height)
                if not row_ok.any():
                    continue
                for a in range(-int(r.max()), int(r.max()) + 1):
                    xx = px + a
                    ok = row_ok & (abs(a) <= r) & (xx >= 0) & (xx < width)
                    if ok.any():
                        np.minimum.at(keys[v], yy[ok] * width + xx[ok], key[ok])
    empty = keys == _EMPTY
    index = np.where(empty, -1, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    depth = np.where(empty, np.float32(np.inf), _ord32_decode((keys >> np.uint64(32)).astype(np.uint32)))
    return index.reshape(n_views, height, width), depth.astype(np.float32).reshape(n_views, height, width), culled


def _buffers_numpy(index, depth):
    index = np.ascontiguousarray(_host(index))
    if index.ndim != 3 or index.dtype != np.int32 or 0 in index.shape:
        raise ValueError('index: an int32 array [V, H, W] of at least one pixel')
    if depth is not None:
        depth = np.ascontiguousarray(_host(depth))
        if depth.shape != index.shape or depth.dtype != np.float32:
            raise ValueError('depth: a float32 array of the shape of index')
    return index, depth


def _colors_numpy(colors):
    colors = np.ascontiguousarray(_host(colors))
    if colors.ndim != 2 or colors.shape[1] != 3 or colors.dtype != np.uint8:
        raise ValueError('colors: a uint8 array [n, 3]')
    return colors


def shade_numpy(index, depth, colors, background=(255, 255, 255), edl=None):
    """index int32 / depth float32 [V, H, W] of ``rasterize``, colors uint8 [n, 3] -> uint8 [V, H, W, 3]"""
    edl, bg = _edl(edl), _background(background)
    index, depth = _buffers_numpy(index, depth if edl is not None else None)
    colors = _colors_numpy(colors)
    owned = index >= 0
    if owned.any() and int(index.max()) >= colors.shape[0]:
        raise ValueError(f'a pixel is owned by point {int(index.max())}: outside the {colors.shape[0]} colours')
    image = np.empty(index.shape + (3,), np.uint8)
    image[...] = np.array(bg, np.uint8)
    image[owned] = colors[index[owned]]
    if edl is None:
        return image
    strength, s, scale = edl
    n_views, height, width = index.shape
    d = depth.astype(np.float64)
    total = np.zeros(index.shape, np.float64)
    count = np.zeros(index.shape, np.int64)
    with np.errstate(all='ignore'):
        for ox, oy in EDL_NEIGHBOURS:
            ox, oy = ox * s, oy * s
            # the pixels (y, x) whose neighbour (y + oy, x + ox) lies inside the image
            y0, y1, x0, x1 = max(0, -oy), min(height, height - oy), max(0, -ox), min(width, width - ox)
            if y0 >= y1 or x0 >= x1:
                continue
            here = (slice(None), slice(y0, y1), slice(x0, x1))
            there = (slice(None), slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
            count[here] += 1
            t = d[here] - d[there]
            t = np.where(t > 0.0, t, 0.0)
            t = t / scale
            t = np.where(t < 1.0, t, 1.0)
            total[here] = total[here] + np.where(owned[there], t, 0.0)
        resp = np.where(count > 0, total / np.maximum(count, 1).astype(np.float64), 0.0)
        factor = 1.0 / (1.0 + strength * resp)
        lit = np.floor(image.astype(np.float64) * factor[..., None] + 0.5).astype(np.uint8)
    image[owned] = lit[owned]
    return image


# ---- the device ------------------------------------------------------------------------------------------------------
def _device_or_numpy(backend, what, n, n_views, width, height):
    chosen = auto_backend(backend, what)
    if chosen == 'device' and not in_device_range(n, n_views, width, height):
        if backend == 'device':
            from .. import _lib as L
            raise L.SoftGroupHipError(f'{what}: {n} points into {n_views} views of {width} x {height}: outside the '
                                      f'supported range (fewer than 2**31 - 1 points, 1 .. {MAX_VIEWS} views, sides '
                                      f'1 .. {MAX_SIDE}, at most 2**26 pixels)')
        chosen = 'numpy'
    return chosen


def rasterize_device(coords, cams, width, height, point_size, world, stages=_STAGE_ALL, buffers=None):
    """``sg_render_rasterize`` on a CUDA float32 tensor [N, 3] and a CUDA camera table; nothing synchronises.
    ``buffers`` = (index, depth, culled, workspace) of an earlier call runs single ``stages`` on them (measurements)."""
    import torch
    from .. import _lib as L
    lib = L.lib()
    dev, n, n_views = coords.device, coords.size(0), cams.size(0)
    with torch.cuda.device(dev):
        if buffers is None:
            buffers = (torch.empty((n_views, height, width), dtype=torch.int32, device=dev),
                       torch.empty((n_views, height, width), dtype=torch.float32, device=dev),
                       torch.empty(n_views, dtype=torch.int32, device=dev),
                       L.workspace(lib.sg_render_rasterize_workspace_bytes(n_views, width, height), dev))
        index, depth, culled, ws = buffers
        L.check(lib.sg_render_rasterize(L.ptr(coords) if n else None, n, L.ptr(cams), n_views, width, height,
                                        point_size, world, stages, L.ptr(index), L.ptr(depth), L.ptr(culled),
                                        L.ptr(ws), ws.numel(), L.stream()), 'sg_render_rasterize')
    return buffers


def rasterize(coords, cameras, width, height, point_size=1, world_radius=None, backend='auto'):
    """-> (index int32 [V, H, W], depth float32 [V, H, W], culled int32 [V]).  A CUDA tensor in gives CUDA tensors
    out (``culled`` is read back only when the caller reads it), numpy in gives numpy out."""
    import torch
    cams = camera_table(cameras)
    width, height = _size(width, height)
    point_size, world = _radius(point_size, world_radius)
    cuda = _is_cuda(coords)
    if torch.is_tensor(coords):
        if coords.dim() != 2 or coords.size(1) != 3:
            raise ValueError('coords: a tensor [n, 3]')
        n = coords.size(0)
    else:
        coords = _xyz_numpy(coords, 'coords')
        n = coords.shape[0]
    if _device_or_numpy(backend, 'rasterize', n, cams.shape[0], width, height) == 'numpy':
        out = rasterize_numpy(_host(coords), cams, width, height, point_size, world_radius)
        return tuple(torch.from_numpy(a).to(coords.device) for a in out) if cuda else out
    # (a CPU tensor goes the way of a numpy array: through the host helper, then one upload)
    xyz = coords.detach().to(torch.float32).contiguous() if cuda else _upload(_xyz_numpy(coords, 'coords'))
    with torch.cuda.device(xyz.device):
        table = torch.from_numpy(cams).to(xyz.device)
    index, depth, culled, _ = rasterize_device(xyz, table, width, height, point_size, world)
    return (index, depth, culled) if cuda else (index.cpu().numpy(), depth.cpu().numpy(), culled.cpu().numpy())


def shade_device(index, depth, colors, bg, edl):
    """``sg_render_shade`` on CUDA tensors -> (image uint8 [V, H, W, 3], flags int32 [1]); nothing synchronises"""
    import torch
    from .. import _lib as L
    dev = index.device
    n_views, height, width = index.shape
    strength, radius, scale = edl if edl is not None else (0.0, 1, 1.0)
    with torch.cuda.device(dev):
        image = torch.empty((n_views, height, width, 3), dtype=torch.uint8, device=dev)
        flags = torch.empty(1, dtype=torch.int32, device=dev)
        L.check(L.lib().sg_render_shade(L.ptr(index), L.ptr(depth), n_views, width, height,
                                        L.ptr(colors) if colors.numel() else None, colors.size(0), bg[0], bg[1], bg[2],
                                        int(edl is not None), strength, radius, scale, L.ptr(image), L.ptr(flags),
                                        L.stream()), 'sg_render_shade')
    return image, flags


def shade(index, depth, colors, background=(255, 255, 255), edl=None, backend='auto'):
    """-> uint8 [V, H, W, 3]; CUDA buffers in give a CUDA image out, numpy in gives numpy out.  ``ValueError`` when
    a pixel is owned by a point outside ``colors`` (on the device after one small read-back)."""
    import torch
    edl, bg = _edl(edl), _background(background)
    cuda = _is_cuda(index)
    shape = tuple(index.shape)
    if len(shape) != 3 or 0 in shape:
        raise ValueError('index: an int32 array [V, H, W] of at least one pixel')
    if _device_or_numpy(backend, 'shade', 0, shape[0], shape[2], shape[1]) == 'numpy':
        image = shade_numpy(index, depth, colors, bg, edl)
        return torch.from_numpy(image).to(index.device) if cuda else image
    if cuda:
        if index.dtype != torch.int32 or (edl is not None and (depth.dtype != torch.float32 or
                                                                tuple(depth.shape) != shape)):
            raise ValueError('index int32 and depth float32, both [V, H, W]')
        d_index, d_depth = index.contiguous(), None if depth is None else depth.to(index.device).contiguous()
    else:
        h_index, h_depth = _buffers_numpy(index, depth if edl is not None else None)
        d_index, d_depth = _upload(h_index), None if h_depth is None else _upload(h_depth)
    if torch.is_tensor(colors):
        if colors.dim() != 2 or colors.size(1) != 3 or colors.dtype != torch.uint8:
            raise ValueError('colors: a uint8 tensor [n, 3]')
        d_colors = colors.detach().to(d_index.device).contiguous()
    else:
        d_colors = _upload(_colors_numpy(colors)).to(d_index.device)
    image, flags = shade_device(d_index, d_depth, d_colors, bg, edl)
    if int(flags.item()) & FLAG_COLOR_INDEX:
        raise ValueError(f'a pixel is owned by a point outside the {d_colors.size(0)} colours')
    return image if cuda else image.cpu().numpy()
