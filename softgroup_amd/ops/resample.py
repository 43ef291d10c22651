"""Thinning a cloud and carrying results back to every original point (csrc/resample.hip): the voxel-grid
downsample, the exact nearest source point, bit-row masks through an index map and bit rows -> runs.

The reference has none of these on the device (dataset/s3dis/downsample.py draws a random sample on the host and
raises for ``--voxel-size``); the rules are this project's and are stated in include/softgroup_hip.h:

* cell of a point, per axis: ``floor(float64(x) / voxel)`` -- one IEEE division; a coordinate that is not finite or
  a cell at or beyond 2**31 raises ``ValueError``;
* representative of a voxel: ``'first'`` the lowest index, ``'center'`` the smallest
  ``d2 = (dx*dx + dy*dy) + dz*dz`` with ``dx = float64(x) - (float64(c) + 0.5) * voxel``, the lowest index among
  equal ``d2``; ``sample_ids`` ascending, ``inverse`` the position of every point's representative in it;
* nearest source: the smallest ``d2 = (dx*dx + dy*dy) + dz*dz`` in float64, the LOWEST source index among equal
  ``d2``; with ``max_dist`` a query farther than that gets -1 (and ``dist2`` +inf); equal to the brute force for
  every query and every ``cell`` -- the grid only decides what the search costs.

CUDA tensors take the HIP kernels, numpy arrays (and CPU tensors) the ``*_numpy`` twins, which obey the same rules.
``nearest_index_numpy`` is the DEFINITION, a chunked O(N x M) brute force, not a fast path.
"""
import ctypes as C

import numpy as np

from ._args import _max_dist, _upload, _words, _xyz_device, _xyz_numpy, choose_backend

__all__ = ['grid_downsample', 'grid_downsample_numpy', 'nearest_index', 'nearest_index_numpy', 'nearest_default_cell',
           'mask_bits_gather', 'mask_bits_gather_numpy', 'mask_runs_from_bits', 'mask_runs_from_bits_numpy',
           'mask_runs_supported', 'auto_backend']

_PICK = {'first': 0, 'center': 1}      # softgroup_hip.h: SG_PICK_*

# what backend='auto' means with a GPU present -- the single place to change.  The nearest point is on the device
# as a matter of feasibility (the numpy path is the O(N x M) definition).  The voxel downsample and the mask
# propagation follow profiles/resample_bench.txt, where the device is ahead on both clouds: 0.15 - 0.26 ms against
# 396 - 1121 ms for the voxels, 1.8 - 5.4 ms against 87 - 421 ms for propagate_result (wall, MI355X).
_AUTO = {'nearest': 'device', 'voxel': 'device', 'masks': 'device'}


def auto_backend(backend, what):
    """'device' or 'numpy' for one of the operations of ``_AUTO``"""
    return choose_backend(backend, _AUTO[what])


def _pick(pick):
    if pick not in _PICK:
        raise ValueError(f"pick {pick!r}: one of 'first', 'center'")
    return _PICK[pick]


def _voxel(voxel):
    voxel = float(voxel)
    if not (voxel > 0.0 and np.isfinite(voxel)):
        raise ValueError(f'voxel size {voxel!r}: a finite number > 0')
    return voxel


# ---- voxel-grid downsample -----------------------------------------------------------------------------------------
def _cells_numpy(xyz, voxel):
    if not np.isfinite(xyz).all():
        raise ValueError('voxel downsample: a coordinate that is not finite')
    c = np.floor(xyz.astype(np.float64) / voxel)
    if c.size and np.abs(c).max() >= 2.0**31:
        raise ValueError('voxel downsample: a cell index at or beyond 2**31 (voxel size too small for the coordinates)')
    return c.astype(np.int64)


def grid_downsample_numpy(xyz, voxel, pick='center'):
    """-> (sample_ids int32 [n_voxels] ascending, inverse int32 [n]) by ``np.unique(axis=0)`` and ``lexsort``"""
    pk, voxel = _pick(pick), _voxel(voxel)
    xyz = _xyz_numpy(xyz)
    n = xyz.shape[0]
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    c = _cells_numpy(xyz, voxel)
    _, vox = np.unique(c, axis=0, return_inverse=True)
    vox = vox.reshape(-1)
    idx = np.arange(n)
    if pk == 0:
        order = np.lexsort((idx, vox))
    else:
        d = xyz.astype(np.float64) - (c.astype(np.float64) + 0.5) * voxel
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        order = np.lexsort((idx, d2, vox))
    head = np.concatenate([[True], vox[order][1:] != vox[order][:-1]])
    rep_of_vox = np.empty(int(vox.max()) + 1, np.int64)
    rep_of_vox[vox[order][head]] = order[head]
    sample_ids = np.sort(rep_of_vox)
    inverse = np.searchsorted(sample_ids, rep_of_vox[vox])
    return sample_ids.astype(np.int32), inverse.astype(np.int32)


def grid_downsample(xyz, voxel, pick='center'):
    """``sg_grid_downsample`` on a CUDA tensor [n, 3] -> (sample_ids int32 [n_voxels] ascending, inverse int32 [n]),
    CUDA.  One read-back of the two meta words (the voxel count and the validity flag).  Other inputs: numpy."""
    import torch
    if not (torch.is_tensor(xyz) and xyz.is_cuda):
        return grid_downsample_numpy(xyz, voxel, pick)
    from .. import _lib as L
    pk, voxel = _pick(pick), _voxel(voxel)
    xyz = _xyz_device(xyz)
    n, dev = xyz.size(0), xyz.device
    lib = L.lib()
    with torch.cuda.device(dev):
        sample_ids = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        inverse = torch.empty(n, dtype=torch.int32, device=dev)
        meta = torch.empty(2, dtype=torch.int32, device=dev)
        ws = L.workspace(lib.sg_grid_downsample_workspace_bytes(n), dev)
        L.check(lib.sg_grid_downsample(L.ptr(xyz) if n else None, n, voxel, pk, L.ptr(sample_ids),
                                       L.ptr(inverse) if n else None, L.ptr(meta), L.ptr(ws), ws.numel(), L.stream()),
                'sg_grid_downsample')
        n_voxels, flags = meta.cpu().tolist()
    if flags:
        raise ValueError('voxel downsample: a coordinate that is not finite, or a cell index at or beyond 2**31 '
                         '(voxel size too small for the coordinates)')
    return sample_ids[:n_voxels], inverse


# ---- nearest source point ------------------------------------------------------------------------------------------
def nearest_default_cell(lo, hi, n_src):
    """``sg_nearest_default_cell``: about two sources per cell of the sources' bounding box [lo, hi]"""
    from .. import _lib as L
    lo = np.ascontiguousarray(lo, dtype=np.float64).reshape(3)
    hi = np.ascontiguousarray(hi, dtype=np.float64).reshape(3)
    return float(L.lib().sg_nearest_default_cell(C.c_void_p(lo.ctypes.data), C.c_void_p(hi.ctypes.data), int(n_src)))


def nearest_index_numpy(src, query, cell=None, max_dist=None, return_dist=False, chunk=1024):
    """The definition: a chunked float64 brute force, O(n_src x n_query) -- feasible for tests and small clouds
    only.  ``cell`` is accepted and ignored (the result does not depend on it).
    -> index int64 [n_query] (and dist2 float64 with ``return_dist``)"""
    src, query = _xyz_numpy(src, 'src'), _xyz_numpy(query, 'query')
    md = _max_dist(max_dist)
    if src.shape[0] < 1:
        raise ValueError('nearest_index: at least one source point')
    if not (np.isfinite(src).all() and np.isfinite(query).all()):
        raise ValueError('nearest_index: a coordinate that is not finite')
    s = src.astype(np.float64)
    index = np.empty(query.shape[0], np.int64)
    dist2 = np.empty(query.shape[0], np.float64)
    for lo in range(0, query.shape[0], chunk):
        q = query[lo:lo + chunk].astype(np.float64)
        dx = q[:, None, 0] - s[None, :, 0]
        d2 = dx * dx
        dx = q[:, None, 1] - s[None, :, 1]
        d2 += dx * dx
        dx = q[:, None, 2] - s[None, :, 2]
        d2 += dx * dx
        j = d2.argmin(1)                            # (the first minimum: the lowest index among equal d2)
        index[lo:lo + chunk] = j
        dist2[lo:lo + chunk] = d2[np.arange(q.shape[0]), j]
    if md >= 0.0:
        far = dist2 > md * md
        index[far] = -1
        dist2[far] = np.inf
    return (index, dist2) if return_dist else index


def nearest_index(src, query, cell=None, max_dist=None, return_dist=False, return_meta=False, backend='auto'):
    """``sg_nearest_build`` + ``sg_nearest_query`` -> index int64 [n_query]: the nearest source of every query,
    exactly (see the module text); ``cell``: the grid's cell size, default ``nearest_default_cell`` of the sources'
    bounding box (one read-back); with ``return_dist`` also dist2 float64; with ``return_meta`` also the number of
    queries the full scan answered.  CUDA tensors in give CUDA tensors out.  numpy arrays (or CPU tensors) in give
    numpy out: through the device when ``backend`` says so (``'auto'``: whenever there is a GPU), else through
    ``nearest_index_numpy``."""
    import torch
    on_device = torch.is_tensor(src) and src.is_cuda
    if not on_device:
        if auto_backend(backend, 'nearest') == 'device':
            out = nearest_index(_upload(_xyz_numpy(src, 'src')), _upload(_xyz_numpy(query, 'query')), cell, max_dist,
                                return_dist, True)
            out = tuple(o.cpu().numpy() if torch.is_tensor(o) else o for o in out)
            out = out if return_meta else out[:-1]
            return out if len(out) > 1 else out[0]
        out = nearest_index_numpy(src, query, cell, max_dist, return_dist)
        return (out + (0, ) if return_dist else (out, 0)) if return_meta else out
    from .. import _lib as L
    md = _max_dist(max_dist)
    src = _xyz_device(src, 'src')
    dev = src.device
    query = _xyz_device(torch.as_tensor(query).to(dev), 'query')
    n_src, n_query = src.size(0), query.size(0)
    if n_src < 1:
        raise ValueError('nearest_index: at least one source point')
    lib = L.lib()
    with torch.cuda.device(dev):
        if cell is None:
            box = torch.stack([src.amin(0), src.amax(0)]).double().cpu().numpy()
            if not np.isfinite(box).all():
                raise ValueError('nearest_index: a coordinate that is not finite')
            cell = nearest_default_cell(box[0], box[1], n_src)
        cell = float(cell)
        if not (cell > 0.0 and np.isfinite(cell)):
            raise ValueError(f'cell {cell!r}: a finite number > 0')
        nb = lib.sg_nearest_grid_bytes(n_src)
        grid = L.workspace(nb, dev)
        meta = torch.empty(2, dtype=torch.int32, device=dev)
        L.check(lib.sg_nearest_build(L.ptr(src), n_src, cell, L.ptr(grid), grid.numel(), L.ptr(meta), L.stream()),
                'sg_nearest_build')
        index = torch.empty(n_query, dtype=torch.int32, device=dev)
        dist2 = torch.empty(n_query, dtype=torch.float64, device=dev) if return_dist else None
        ws = L.workspace(lib.sg_nearest_query_workspace_bytes(n_query), dev)
        L.check(lib.sg_nearest_query(L.ptr(src), n_src, cell, L.ptr(grid), grid.numel(), L.ptr(query) if n_query else None,
                                     n_query, md, L.ptr(index) if n_query else None,
                                     L.ptr(dist2) if (return_dist and n_query) else None, L.ptr(meta), L.ptr(ws),
                                     ws.numel(), L.stream()), 'sg_nearest_query')
        scanned, flags = meta.cpu().tolist()
    if flags & 3:
        raise ValueError('nearest_index: a coordinate that is not finite')
    out = (index.long(), dist2) if return_dist else (index.long(), )
    if return_meta:
        out = out + (scanned, )
    return out if len(out) > 1 else out[0]


# ---- masks -----------------------------------------------------------------------------------------------------------
def mask_bits_gather_numpy(bits, n_src, index):
    """packed rows (any integer dtype, [n, >= ceil(n_src / 8)] bytes, little-endian bit order) through ``index``
    -> uint8 [n, 4 * ceil(n_out / 32)], the bytes of the gathered bit rows (``unpackbits``, a take, ``packbits``)"""
    bits = np.ascontiguousarray(bits)
    n = bits.shape[0]
    rows = bits.view(np.uint8).reshape(n, -1)
    index = np.asarray(index).reshape(-1).astype(np.int64)
    if index.size and index.max() >= n_src:
        raise ValueError(f'mask_bits_gather: an index >= {n_src}')
    n_out = index.size
    out = np.zeros((n, _words(n_out) * 4), dtype=np.uint8)
    if n == 0 or n_out == 0:
        return out
    dense = np.unpackbits(rows, axis=1, count=None, bitorder='little')[:, :n_src] if n_src else np.zeros((n, 0), np.uint8)
    got = np.zeros((n, n_out), dtype=np.uint8)
    ok = index >= 0
    got[:, ok] = dense[:, index[ok]]
    p = np.packbits(got, axis=1, bitorder='little')
    out[:, :p.shape[1]] = p
    return out


def mask_bits_gather(bits, n_src, index, check=False):
    """``sg_mask_bits_gather``: CUDA bit rows int32 [n, ceil(n_src / 32)] and a CUDA integer ``index`` [n_out]
    (-1 = no source) -> int32 [n, ceil(n_out / 32)]: bit i of row k = bit index[i] of source row k.  Other inputs:
    numpy.

    An index >= n_src is the caller's error, and the two paths differ on it unless ``check`` is set: the numpy path
    always raises ``ValueError``; the device path never reads out of bounds, and by default (``check=False``,
    nothing synchronises) treats such an index as -1 without a word.  With ``check=True`` it reads the kernel's
    flag word back (one synchronisation) and raises ``ValueError`` too."""
    import torch
    if not (torch.is_tensor(bits) and bits.is_cuda):
        if torch.is_tensor(bits):
            bits = bits.numpy()
        if torch.is_tensor(index):
            index = index.cpu().numpy()
        return mask_bits_gather_numpy(bits, n_src, index)
    from .. import _lib as L
    n_src = int(n_src)
    if bits.dim() != 2 or bits.element_size() != 4 or bits.is_floating_point() or bits.size(1) != _words(n_src):
        raise ValueError(f'bits: an integer tensor [n, {_words(n_src)}] of 32-bit words')
    dev = bits.device
    bits = bits.contiguous()
    index = torch.as_tensor(index).to(dev, torch.int32).reshape(-1).contiguous()
    n, n_out = bits.size(0), index.numel()
    with torch.cuda.device(dev):
        out = torch.empty((n, _words(n_out)), dtype=torch.int32, device=dev)
        meta = torch.empty(1, dtype=torch.int32, device=dev) if check else None
        L.check(L.lib().sg_mask_bits_gather(L.ptr(bits) if bits.numel() else None, n, n_src,
                                            L.ptr(index) if n_out else None, n_out, L.ptr(out) if out.numel() else None,
                                            L.ptr(meta) if check else None, L.stream()), 'sg_mask_bits_gather')
        if check and int(meta.item()):
            raise ValueError(f'mask_bits_gather: an index >= {n_src}')
    return out


def mask_runs_from_bits_numpy(bits, n_points):
    """packed rows -> (starts int32, ends int32, bounds int64 [n + 1]): the maximal runs of every row, 0-based,
    end exclusive, ascending (``unpackbits`` and ``np.diff``)"""
    bits = np.ascontiguousarray(bits)
    n = bits.shape[0]
    rows = bits.view(np.uint8).reshape(n, -1)
    n_points = int(n_points)
    dense = np.unpackbits(rows, axis=1, bitorder='little')[:, :n_points] if n_points else np.zeros((n, 0), np.uint8)
    pad = np.zeros((n, n_points + 2), dtype=np.int8)
    pad[:, 1:-1] = dense
    edge = np.diff(pad, axis=1)
    r_s, c_s = np.nonzero(edge == 1)
    _, c_e = np.nonzero(edge == -1)
    bounds = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r_s, minlength=n), out=bounds[1:])
    return c_s.astype(np.int32), c_e.astype(np.int32), bounds


def mask_runs_supported(n, n_points):
    """whether ``n`` masks over ``n_points`` points are inside the device's range (its run numbers are int32:
    ``n * ceil(n_points / 2) < 2**31``) -- the rule of ``sg_mask_runs_workspace_bytes``, asked of the library"""
    from .. import _lib as L
    return 0 <= int(n) < 2**31 and 0 <= int(n_points) < 2**63 and \
        L.lib().sg_mask_runs_workspace_bytes(int(n), int(n_points)) != 0


def mask_runs_from_bits(bits, n_points):
    """``sg_mask_runs_count`` + ``sg_mask_runs_fill``: CUDA bit rows int32 [n, ceil(n_points / 32)] -> (starts int32,
    ends int32, bounds int64 [n + 1]) on the device, what ``sg_rle_format_device`` and ``mask_bits_from_runs`` take.
    One read-back (the run total) between the passes.  Other inputs: numpy."""
    import torch
    if not (torch.is_tensor(bits) and bits.is_cuda):
        return mask_runs_from_bits_numpy(bits.numpy() if torch.is_tensor(bits) else bits, n_points)
    from .. import _lib as L
    n_points = int(n_points)
    if bits.dim() != 2 or bits.element_size() != 4 or bits.is_floating_point() or bits.size(1) != _words(n_points):
        raise ValueError(f'bits: an integer tensor [n, {_words(n_points)}] of 32-bit words')
    dev = bits.device
    bits = bits.contiguous()
    n = bits.size(0)
    lib = L.lib()
    with torch.cuda.device(dev):
        nb = lib.sg_mask_runs_workspace_bytes(n, n_points)
        if nb == 0:
            raise L.SoftGroupHipError(f'mask_runs_from_bits: {n} masks over {n_points} points: outside the supported '
                                      'range (n * ceil(n_points / 2) < 2**31)')
        ws = L.workspace(nb, dev)
        bounds = torch.empty(n + 1, dtype=torch.int64, device=dev)
        b = L.ptr(bits) if bits.numel() else None
        L.check(lib.sg_mask_runs_count(b, n, n_points, L.ptr(bounds), L.ptr(ws), ws.numel(), L.stream()),
                'sg_mask_runs_count')
        total = int(bounds[n].item())
        starts = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        ends = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        L.check(lib.sg_mask_runs_fill(b, n, n_points, L.ptr(ws), ws.numel(), L.ptr(starts), L.ptr(ends), total,
                                      L.stream()), 'sg_mask_runs_fill')
    return starts[:total], ends[:total], bounds
