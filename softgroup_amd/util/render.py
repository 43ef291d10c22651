"""Pictures of a result cloud without a desktop: cameras fitted to the cloud, ``render_cloud`` (coloured points to
uint8 images, ``ops.render``: a z-buffered splat and optional eye-dome lighting), ``render_result`` for a
``forward_test`` result dict, ``save_renders`` for the tree ``save_results`` wrote, and a PNG writer / reader from
``zlib`` alone.  The reference has no counterpart: its docs send the user to MeshLab or PyVista.

Cameras are host code for both backends (``np.sin`` / ``np.cos`` once); the rules of the rasterisation and of the
shading, the device range and the backend rule are in ``ops/render.py`` and include/softgroup_hip.h.  The index image
(which point owns which pixel) is kept between the tasks of a scan: one rasterisation serves every task that shares
the input coordinates, only the colour lookup differs.
"""
import os
import os.path as osp
import struct
import zlib

import numpy as np

from ..ops import render as RO
from ..ops._args import _host, _is_cuda
from ..ops.render import Camera
from . import visualize as V

__all__ = ['Camera', 'VIEWS', 'look_at', 'fit_view', 'named_view', 'turntable', 'cloud_bounds', 'cameras_for',
           'render_cloud', 'render_result', 'save_renders', 'write_png', 'read_png', 'montage']

# name -> (azimuth, elevation) in degrees: where the eye stands, seen from the centre of the box (azimuth from +x
# towards +y, elevation from the xy plane towards +z)
VIEWS = {'top': (-90.0, 90.0), 'front': (-90.0, 0.0), 'side': (0.0, 0.0), 'iso': (-60.0, 30.0)}
_EDL_DEFAULT = (1.0, 1)                   # strength, radius of edl=True; the scale is 1 % of the box diagonal


# ---- cameras -----------------------------------------------------------------------------------------------------
def look_at(eye, target, up=(0, 0, 1)):
    """-> float64 [3, 3] with rows (right, up, forward): forward from ``eye`` to ``target``, right = forward x up.
    Raises when the two points coincide or ``up`` is parallel to the view."""
    eye, target, up = (np.asarray(v, np.float64).reshape(3) for v in (eye, target, up))
    forward = target - eye
    length = np.sqrt((forward * forward).sum())
    if not (length > 0 and np.isfinite(length)):
        raise ValueError('look_at: eye and target are two different finite points')
    forward = forward / length
    right = np.cross(forward, up)
    length = np.sqrt((right * right).sum())
    if not length > 1e-9 * np.sqrt((up * up).sum()) or not np.isfinite(length):
        raise ValueError('look_at: up is parallel to the view')
    right = right / length
    return np.stack([right, np.cross(right, forward), forward])


def _angles(view):
    if isinstance(view, str):
        if view not in VIEWS:
            raise ValueError(f'view {view!r}: one of {", ".join(VIEWS)}, or (azimuth, elevation) in degrees')
        return VIEWS[view]
    azimuth, elevation = view
    return float(azimuth), float(elevation)


def fit_view(lo, hi, azimuth, elevation, size, kind='perspective', fov=50.0, margin=0.05):
    """A camera that looks at the centre of the box ``lo .. hi`` from (azimuth, elevation) degrees and shows every
    point of the box inside the image ``size`` = (width, height): the box's bounding sphere fits the smaller side
    less ``margin`` of it on either side.  ``fov`` is the vertical field of view of a perspective camera, degrees."""
    lo, hi = (np.asarray(v, np.float64).reshape(3) for v in (lo, hi))
    width, height = RO._size(*size)
    if kind not in ('perspective', 'orthographic'):
        raise ValueError(f"kind {kind!r}: 'perspective' or 'orthographic'")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
        raise ValueError('fit_view: a finite box with hi >= lo')
    if not 0 <= margin < 0.5 or not 0 < fov < 180:
        raise ValueError('fit_view: 0 <= margin < 0.5 and 0 < fov < 180')
    centre = (lo + hi) * 0.5
    radius = 0.5 * np.sqrt(((hi - lo) ** 2).sum())
    radius = radius if radius > 0 else 1.0
    az, el = np.deg2rad(azimuth), np.deg2rad(elevation)
    out = np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])      # centre -> eye
    up = np.array([-np.sin(el) * np.cos(az), -np.sin(el) * np.sin(az), np.cos(el)])     # d(out) / d(elevation)
    # half the usable side, half a pixel kept free so that floor() stays below the side
    half = max(min(width, height) * (0.5 - margin) - 0.5, 0.25)
    cx, cy = width * 0.5, height * 0.5
    if kind == 'orthographic':
        eye = centre + out * (2.0 * radius)
        return Camera(kind, eye, look_at(eye, centre, up), half / radius, cx, cy, None, None)
    f = (height * 0.5) / np.tan(np.deg2rad(fov) * 0.5)
    dist = radius / np.sin(np.arctan(half / f))              # the sphere's tangent cone meets the image at `half`
    eye = centre + out * dist
    return Camera(kind, eye, look_at(eye, centre, up), f, cx, cy, (dist - radius) * 0.5, None)


def named_view(name, lo, hi, size, **kw):
    azimuth, elevation = _angles(name)
    return fit_view(lo, hi, azimuth, elevation, size, **kw)


def turntable(n, elevation=30.0, start=-90.0):
    """n (azimuth, elevation) pairs around the cloud, usable wherever a view name is"""
    if isinstance(n, bool) or int(n) != n or int(n) < 1:
        raise ValueError(f'turntable: {n!r} views: an integer >= 1')
    return [(start + 360.0 * k / int(n), float(elevation)) for k in range(int(n))]


def cloud_bounds(xyz):
    """(lo, hi) float64 [3] over the finite points; a CUDA cloud costs one small read-back.  Raises without one."""
    if _is_cuda(xyz):
        import torch
        p = xyz.detach().to(torch.float32)
        ok = torch.isfinite(p).all(1, keepdim=True)
        inf = torch.tensor(float('inf'), device=p.device)
        both = torch.stack([torch.where(ok, p, inf).amin(0), torch.where(ok, p, -inf).amax(0)]) if p.size(0) else \
            torch.stack([inf.expand(3), -inf.expand(3)])
        lo, hi = both.cpu().numpy().astype(np.float64)
    else:
        p = np.asarray(_host(xyz), np.float32).reshape(-1, 3)
        p = p[np.isfinite(p).all(1)]
        lo, hi = (p.min(0), p.max(0)) if len(p) else (np.full(3, np.inf), np.full(3, -np.inf))
        lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError('the cloud has no finite point')
    return lo, hi


def cameras_for(views, lo, hi, size, kind='perspective', fov=50.0, margin=0.05):
    """views: names of ``VIEWS``, (azimuth, elevation) pairs or ready ``Camera``s -> a list of cameras"""
    if isinstance(views, (str, Camera)):
        views = [views]
    return [v if isinstance(v, Camera) else named_view(v, lo, hi, size, kind=kind, fov=fov, margin=margin)
            for v in views]


# ---- rendering ---------------------------------------------------------------------------------------------------
def _edl_params(edl, lo, hi):
    if edl is None or edl is False:
        return None
    if edl is True:
        edl = {}
    if isinstance(edl, dict):
        diagonal = float(np.sqrt(((hi - lo) ** 2).sum()))
        scale = edl.get('scale', 0.01 * diagonal if diagonal > 0 else 1.0)
        edl = (edl.get('strength', _EDL_DEFAULT[0]), edl.get('radius', _EDL_DEFAULT[1]), scale)
    return RO._edl(edl)


def _as_uint8(rgb):
    """colours in 0 .. 255 of any dtype -> uint8 (truncated, clipped); a uint8 array or tensor is taken as it is"""
    import torch
    if torch.is_tensor(rgb):
        if rgb.dtype == torch.uint8:
            return rgb
        rgb = rgb.detach().cpu().numpy()
    rgb = np.asarray(rgb)
    if rgb.dtype == np.uint8:
        return rgb
    if rgb.dtype.kind == 'f':
        rgb = np.trunc(np.nan_to_num(rgb.astype(np.float64), nan=0.0, posinf=255.0, neginf=0.0))
    return np.clip(rgb, 0, 255).astype(np.uint8)


def _like(a, cuda, device):
    """an array or tensor as what the caller handed in: a CUDA tensor on ``device``, or numpy"""
    import torch
    if cuda:
        return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return a.cpu().numpy() if torch.is_tensor(a) else a


def render_cloud(xyz, rgb, views=('iso',), size=(1024, 768), point_size=1, world_radius=None,
                 background=(255, 255, 255), edl=None, backend='auto', kind='perspective', fov=50.0, margin=0.05,
                 return_buffers=False):
    """Coloured points -> uint8 [V, H, W, 3], one image per view (``size`` = (width, height)).  ``xyz`` [N, 3],
    ``rgb`` [N, 3] in 0 .. 255.  CUDA in gives CUDA out (the cloud is not copied to the host), numpy in gives numpy
    out.  ``edl``: None, True (strength 1, radius 1, scale = 1 % of the box diagonal), a dict of those, or the
    triple.  ``return_buffers=True`` -> (image, index, depth)."""
    width, height = RO._size(*size)
    cuda = _is_cuda(xyz)
    device = xyz.device if cuda else None
    lo, hi = cloud_bounds(xyz)
    cams = cameras_for(views, lo, hi, (width, height), kind, fov, margin)
    edl = _edl_params(edl, lo, hi)
    colors = _as_uint8(rgb)
    n = xyz.shape[0]
    if colors.shape[0] != n or colors.ndim != 2 or colors.shape[1] != 3:
        raise ValueError(f'rgb: [{n}, 3], one colour per point')
    index, depth, _ = RO.rasterize(xyz, cams, width, height, point_size, world_radius, backend)
    image = RO.shade(index, depth, _like(colors, cuda, device), background, edl, backend)
    return (image, index, depth) if return_buffers else image


def render_result(result, task='instance_pred', views=('iso',), size=(1024, 768), point_size=1, world_radius=None,
                  background=(255, 255, 255), edl=None, backend='auto', instance_palette=None, class_palette=None,
                  **kw):
    """The picture of one task of a ``forward_test`` result dict: coordinates and colours from
    ``colors_from_result`` (a lazy result resolves there; the two palettes as in ``util/visualize.py``), then
    ``render_cloud``.  -> uint8 numpy [V, H, W, 3]"""
    xyz, rgb = V.colors_from_result(result, task, instance_palette=instance_palette, class_palette=class_palette)
    return render_cloud(np.ascontiguousarray(xyz, np.float32), rgb, views, size, point_size, world_radius, background,
                        edl, backend, **kw)


def save_renders(prediction_path, scan_ids, tasks, out_dir, views=('iso',), size=(1024, 768), point_size=1,
                 world_radius=None, background=(255, 255, 255), edl=None, backend='auto', instance_palette=None,
                 class_palette=None, kind='perspective', fov=50.0, margin=0.05):
    """``<out_dir>/<scan>_<task>.png`` for every scan and task of a ``save_results`` tree, the views side by side.
    Per scan the cloud is rasterised ONCE for all tasks that share the input coordinates (every task but
    ``offset_semantic_pred``) and shaded once per task.  Returns one dict per file: ``path``, ``task``, ``views``,
    ``size`` (of the file), ``points`` and ``rasterized`` (whether this file needed a rasterisation of its own)."""
    for task in tasks:
        if task not in V.TASKS:
            raise ValueError(f'task {task!r}: one of {", ".join(V.TASKS)}')
    width, height = RO._size(*size)
    inst_table = V._palette(instance_palette, V.INSTANCE_PALETTE)
    class_table = V._palette(class_palette, V.SCANNET_CLASS_PALETTE)
    raster = RO.auto_backend(backend, 'rasterize')
    os.makedirs(out_dir, exist_ok=True)
    infos = []
    for room in scan_ids:
        scan = V._file_scan(prediction_path, room, 'numpy')
        shared = None
        for task in tasks:
            xyz, rgb = V._cloud(scan, task, 'numpy', None, inst_table, class_table)
            xyz = np.ascontiguousarray(xyz, np.float32)
            own = task == 'offset_semantic_pred' or shared is None
            if own:
                lo, hi = cloud_bounds(xyz)
                cams = cameras_for(views, lo, hi, (width, height), kind, fov, margin)
                if raster == 'device':
                    from ..ops._args import _upload
                    xyz = _upload(xyz)
                buffers = RO.rasterize(xyz, cams, width, height, point_size, world_radius, backend)[:2] + \
                    (_edl_params(edl, lo, hi), len(cams))
                if task != 'offset_semantic_pred':
                    shared = buffers
            index, depth, edl_p, n_views = buffers if own else shared
            colors = _as_uint8(rgb)
            image = RO.shade(index, depth, _like(colors, _is_cuda(index), getattr(index, 'device', None)), background,
                             edl_p, backend)
            image = _like(image, False, None)
            path = osp.join(out_dir, f'{room}_{task}.png')
            sheet = montage(image, n_views)
            write_png(path, sheet)
            infos.append(dict(path=path, task=task, views=n_views, size=(sheet.shape[1], sheet.shape[0]),
                              points=len(colors), rasterized=bool(own)))
    return infos


# ---- images ------------------------------------------------------------------------------------------------------
_PNG_MAGIC = b'\x89PNG\r\n\x1a\n'


def _chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xFFFFFFFF)


def write_png(path, image, level=6):
    """uint8 [H, W, 3] -> an 8-bit RGB PNG, non-interlaced, filter 0 on every row (``zlib`` and nothing else)"""
    image = np.ascontiguousarray(_host(image))
    if image.ndim != 3 or image.shape[2] != 3 or image.dtype != np.uint8 or 0 in image.shape:
        raise ValueError('write_png: a uint8 image [H, W, 3] of at least one pixel')
    height, width = image.shape[:2]
    rows = np.zeros((height, 1 + 3 * width), np.uint8)                       # (the leading 0 is the filter type)
    rows[:, 1:] = image.reshape(height, 3 * width)
    data = _PNG_MAGIC + _chunk(b'IHDR', struct.pack('>IIBBBBB', width, height, 8, 2, 0, 0, 0)) + \
        _chunk(b'IDAT', zlib.compress(rows.tobytes(), level)) + _chunk(b'IEND', b'')
    with open(path, 'wb') as f:
        f.write(data)
    return len(data)


def read_png(path):
    """the files ``write_png`` writes -> uint8 [H, W, 3]; anything else (another colour type or bit depth, interlace,
    a row filter, a broken checksum) raises ``ValueError``"""
    with open(path, 'rb') as f:
        data = f.read()
    if data[:8] != _PNG_MAGIC:
        raise ValueError(f'{path}: not a PNG file')
    at, header, parts, ended = 8, None, [], False
    while at + 12 <= len(data) and not ended:
        length, = struct.unpack('>I', data[at:at + 4])
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + length]
        crc = data[at + 8 + length:at + 12 + length]
        if len(body) != length or len(crc) != 4 or struct.unpack('>I', crc)[0] != zlib.crc32(kind + body) & 0xFFFFFFFF:
            raise ValueError(f'{path}: a broken chunk')
        if kind == b'IHDR':
            header = struct.unpack('>IIBBBBB', body)
        elif kind == b'IDAT':
            parts.append(body)
        elif kind == b'IEND':
            ended = True
        else:                                                                 # (PLTE among them)
            raise ValueError(f'{path}: chunk {kind.decode("latin1")} is outside the subset write_png writes')
        at += 12 + length
    if header is None or not ended:
        raise ValueError(f'{path}: no header or no end')
    width, height, depth, colour, compression, filtering, interlace = header
    if (depth, colour, compression, filtering, interlace) != (8, 2, 0, 0, 0) or not width or not height:
        raise ValueError(f'{path}: not 8-bit RGB without interlace (bit depth {depth}, colour type {colour}, '
                         f'interlace {interlace})')
    raw = np.frombuffer(zlib.decompress(b''.join(parts)), np.uint8)
    if raw.size != height * (1 + 3 * width):
        raise ValueError(f'{path}: {raw.size} bytes of pixels for {width} x {height}')
    rows = raw.reshape(height, 1 + 3 * width)
    if rows[:, 0].any():
        raise ValueError(f'{path}: a row filter other than 0')
    return rows[:, 1:].reshape(height, width, 3).copy()


def montage(images, cols, background=(255, 255, 255)):
    """uint8 [K, H, W, 3] (or a list of [H, W, 3] of one size) -> one image of ``cols`` columns, row by row; cells
    without an image get the background"""
    images = np.stack([np.asarray(_host(i)) for i in images]) if not hasattr(images, 'shape') else \
        np.asarray(_host(images))
    if images.ndim != 4 or images.shape[3] != 3 or images.dtype != np.uint8 or images.shape[0] < 1:
        raise ValueError('montage: uint8 images [K, H, W, 3], K >= 1')
    if isinstance(cols, bool) or int(cols) != cols or int(cols) < 1:
        raise ValueError(f'montage: {cols!r} columns: an integer >= 1')
    k, height, width = images.shape[:3]
    cols = min(int(cols), k)
    rows = (k + cols - 1) // cols
    sheet = np.empty((rows * height, cols * width, 3), np.uint8)
    sheet[...] = np.array(RO._background(background), np.uint8)
    for j in range(k):
        r, c = divmod(j, cols)
        sheet[r * height:(r + 1) * height, c * width:(c + 1) * width] = images[j]
    return sheet
