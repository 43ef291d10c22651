"""Geometry for clouds that ship no superpoints (csrc/geometry.hip): the exact k nearest neighbours (``sg_knn``),
normal and curvature per point (``sg_point_normals``) and the connected components of "same smooth surface" links
(``sg_grow_segments``).  ``softgroup_amd.util.make_superpoints`` composes the three.

The reference has none of these; the rules are this project's, stated in include/softgroup_hip.h, and the
``*_numpy`` functions are the definition:

* ``knn``: ``d2 = (dx*dx + dy*dy) + dz*dz`` in float64 from the float32 coordinates; the neighbours of point i are
  the k points ``j != i`` with the smallest ``(d2, j)`` in lexicographic order, in that order (equal coordinates: a
  neighbour at distance 0; ties at the k-th place: the lower index); with ``max_dist`` a candidate with
  ``d2 > max_dist * max_dist`` is no neighbour; missing entries are ``-1`` / ``+inf``.  The result does not depend
  on ``cell``, which only decides what the search costs.  ``knn_numpy`` is a chunked O(N x N) brute force, not a
  fast path.
* ``point_normals``: support = the point, then its valid neighbours in list order; centroid and the six covariance
  sums in float64 in that order; normal = unit eigenvector of the smallest eigenvalue, the component of greatest
  magnitude positive (the lowest axis among equal magnitudes); curvature ``max(l0, 0) / (l0 + l1 + l2)``; no normal
  -- ``(0, 0, 0)`` and curvature 0 -- with fewer than ``min_neighbours`` valid neighbours or a covariance trace
  that is not in ``(0, inf)``.  The twin solves with ``np.linalg.eigh``, the device with Jacobi sweeps: the one
  operation here that is not byte-exact.
* ``grow_segments``: an entry j of point i's list links i and j when both have a normal,
  ``abs((nx_i*nx_j + ny_i*ny_j) + nz_i*nz_j) >= cos(radians(angle))`` in float64 from the float32 normals, with
  ``max_curvature`` both curvatures ``<= max_curvature`` (float32), with ``max_dist`` the listed
  ``d2 <= max_dist * max_dist``.  Segments = connected components; those of at least ``min_size`` points are
  numbered in ascending order of their smallest point; the other points get ``-1`` (``small='drop'``) or the number
  of the first entry of their own list that lies in a numbered component (``small='absorb'``, one pass over the
  labels from before the pass).

CUDA tensors in give CUDA tensors out.  numpy arrays (or CPU tensors) in give numpy out, through the device or the
twin as ``backend`` says.
"""
import ctypes as C
import math

import numpy as np

from ._args import _host, _is_cuda, _max_dist, _upload, _xyz_device, _xyz_numpy, choose_backend

__all__ = ['knn', 'knn_numpy', 'knn_default_cell', 'point_normals', 'point_normals_numpy', 'grow_segments',
           'grow_segments_numpy', 'auto_backend', 'MAX_K', 'MAX_SHELL', 'MAX_LISTED']

MAX_K = 32                                # softgroup_hip.h: SG_KNN_MAX_K
MAX_SHELL = 3                             # softgroup_hip.h: SG_KNN_MAX_SHELL
MAX_LISTED = 4096                         # entries per neighbour list on the device (normals, growth)
_FLAG_NOT_FINITE, _FLAG_CELL_RANGE = 1, 4
_FLAG_INDEX, _FLAG_INTERNAL = 1, 2

# what backend='auto' means with a GPU present -- the single place to change.  Set from
# profiles/geometry_bench.txt (tools/geometry_bench.py, MI355X; clouds of 150 k and 600 k points, k = 8 .. 32), where
# the device is ahead on every row: the normals 0.07 - 1.1 ms against 171 - 2462 ms, the growth 1.5 - 15 ms against
# 74 - 1569 ms.  knn is on the device as a matter of feasibility (the numpy path is the O(N x N) definition), like
# nearest_index: 0.9 - 17 ms, against 56 - 297 ms of scipy's cKDTree on 16 threads, which is not tie-exact.
_AUTO = {'knn': 'device', 'normals': 'device', 'grow': 'device'}


def auto_backend(backend, what):
    """'device' or 'numpy' for one of the operations of ``_AUTO``"""
    return choose_backend(backend, _AUTO[what])


def _k(k):
    if int(k) != k or not 1 <= int(k) <= MAX_K:
        raise ValueError(f'k {k!r}: an integer in 1 .. {MAX_K}')
    return int(k)


def _cell(cell):
    cell = float(cell)
    if not (cell > 0.0 and np.isfinite(cell)):
        raise ValueError(f'cell {cell!r}: a finite number > 0')
    return cell


def _bad_xyz(flags=_FLAG_NOT_FINITE):
    if flags & _FLAG_NOT_FINITE:
        return ValueError('knn: a coordinate that is not finite')
    return ValueError('knn: a cell index at or beyond 2**30 (cell too small for the coordinates)')


# ---- k nearest neighbours ------------------------------------------------------------------------------------------
def knn_default_cell(lo, hi, n, k):
    """``sg_knn_default_cell``: about k / 2 points per cell were the cloud spread evenly over its bounding box
    [lo, hi] -- ``(max(k, 2) / 2 * volume / n) ** (1 / D)`` over the D extents that are > 0, and at least
    ``max|coordinate| / 2**29``.  Scanned clouds are surfaces and denser than that where they have points: the k-th
    neighbour then lies inside one cell and the walk ends after the first shell."""
    from .. import _lib as L
    lo = np.ascontiguousarray(lo, dtype=np.float64).reshape(3)
    hi = np.ascontiguousarray(hi, dtype=np.float64).reshape(3)
    return float(L.lib().sg_knn_default_cell(C.c_void_p(lo.ctypes.data), C.c_void_p(hi.ctypes.data), int(n), int(k)))


def knn_numpy(xyz, k, cell=None, max_dist=None, chunk=32):
    """The definition: a chunked float64 brute force with a stable sort of ``d2`` (= the order of ``(d2, j)``).
    ``cell`` is checked like the device checks it and otherwise ignored.
    -> (idx int32 [n, k], d2 float64 [n, k])"""
    k, md = _k(k), _max_dist(max_dist)
    xyz = _xyz_numpy(xyz)
    n = xyz.shape[0]
    if not np.isfinite(xyz).all():
        raise _bad_xyz()
    if cell is not None and n and np.abs(np.floor(xyz.astype(np.float64) / _cell(cell))).max() >= 2.0**30:
        raise _bad_xyz(_FLAG_CELL_RANGE)
    idx = np.full((n, k), -1, np.int32)
    dist = np.full((n, k), np.inf, np.float64)
    p = xyz.astype(np.float64)
    kk = min(k, max(n - 1, 0))
    for lo in range(0, n, chunk):
        q = p[lo:lo + chunk]
        dx = q[:, None, 0] - p[None, :, 0]
        d2 = dx * dx
        dx = q[:, None, 1] - p[None, :, 1]
        d2 += dx * dx
        dx = q[:, None, 2] - p[None, :, 2]
        d2 += dx * dx
        d2[np.arange(q.shape[0]), np.arange(lo, lo + q.shape[0])] = np.inf      # j != i
        if md >= 0.0:
            d2[d2 > md * md] = np.inf
        if kk == 0:
            continue
        # kk smallest by value (any of those that tie with the kk-th), ascending j, then a stable sort by d2: the
        # order of (d2, j) -- for the rows where nothing outside the selection ties with the kk-th
        part = np.sort(np.argpartition(d2, kk - 1, axis=1)[:, :kk], axis=1)
        dpart = np.take_along_axis(d2, part, 1)
        order = np.argsort(dpart, axis=1, kind='stable')
        part, dpart = np.take_along_axis(part, order, 1), np.take_along_axis(dpart, order, 1)
        kth = dpart[:, -1]
        fine = np.isfinite(kth) & ((d2 <= kth[:, None]).sum(1) == kk)
        rows = np.flatnonzero(fine)
        idx[lo + rows, :kk] = part[rows]
        dist[lo + rows, :kk] = dpart[rows]
        for r in np.flatnonzero(~fine):                     # ties at the kk-th place, or fewer than kk candidates
            cand = np.flatnonzero(d2[r] <= kth[r])
            cand = cand[np.isfinite(d2[r, cand])]
            best = cand[np.argsort(d2[r, cand], kind='stable')][:kk]
            idx[lo + r, :best.size] = best
            dist[lo + r, :best.size] = d2[r, best]
    return idx, dist


def _knn_device(xyz, k, cell, md, return_meta):
    import torch

    from .. import _lib as L
    xyz = _xyz_device(xyz)
    n, dev = xyz.size(0), xyz.device
    lib = L.lib()
    with torch.cuda.device(dev):
        idx = torch.empty((n, k), dtype=torch.int32, device=dev)
        d2 = torch.empty((n, k), dtype=torch.float64, device=dev)
        if n == 0:
            return (idx, d2, 0) if return_meta else (idx, d2)
        checked = False
        if cell is None:
            # the one read-back of the call: the box decides the cell, shows a coordinate that is not finite (amin /
            # amax carry a NaN) and, by the cell's lower bound, keeps every cell index inside the grid's range
            box = torch.stack([xyz.amin(0), xyz.amax(0)]).double().cpu().numpy()
            if not np.isfinite(box).all():
                raise _bad_xyz()
            cell = knn_default_cell(box[0], box[1], n, k)
            checked = True
        cell = _cell(cell)
        nb = lib.sg_knn_workspace_bytes(n, k)
        if nb == 0:
            raise L.SoftGroupHipError(f'knn: {n} points, k {k}: outside the supported range')
        ws = L.workspace(nb, dev)
        meta = torch.empty(4, dtype=torch.int32, device=dev)
        L.check(lib.sg_knn(L.ptr(xyz), n, k, cell, md, L.ptr(idx), L.ptr(d2), L.ptr(meta), L.ptr(ws), ws.numel(),
                           L.stream()), 'sg_knn')
        scanned = 0
        if not checked or return_meta:
            scanned, flags = meta[:2].cpu().tolist()
            if flags:
                raise _bad_xyz(flags)
    return (idx, d2, scanned) if return_meta else (idx, d2)


def knn(xyz, k, cell=None, max_dist=None, backend='auto', return_meta=False):
    """``sg_knn`` -> (idx int32 [n, k], d2 float64 [n, k]): the k nearest other points of every point, exactly (see
    the module text).  ``cell``: the grid's cell size, a speed knob only; ``None`` takes ``knn_default_cell`` of the
    bounding box, which costs the call's one read-back (with a ``cell`` the read-back is that of the flags).  With
    ``return_meta`` also the number of queries the full scan answered.  A coordinate that is not finite, or a cell
    index at or beyond 2**30, raises ``ValueError``."""
    k, md = _k(k), _max_dist(max_dist)
    if cell is not None:
        cell = _cell(cell)
    if _is_cuda(xyz):
        auto_backend(backend, 'knn')
        return _knn_device(xyz, k, cell, md, return_meta)
    if auto_backend(backend, 'knn') == 'device':
        out = _knn_device(_upload(_xyz_numpy(xyz)), k, cell, md, return_meta)
        return tuple(o.cpu().numpy() if hasattr(o, 'cpu') else o for o in out)
    out = knn_numpy(xyz, k, cell, max_dist)
    return out + (0, ) if return_meta else out


# ---- normals ---------------------------------------------------------------------------------------------------------
def _nbr_numpy(nbr_idx, n):
    nbr = _host(nbr_idx)
    if nbr.ndim != 2 or nbr.dtype.kind not in 'iu' or nbr.shape[0] != n or nbr.shape[1] < 1:
        raise ValueError(f'nbr_idx: an integer array [{n}, k], k >= 1')
    if nbr.size and (int(nbr.min()) < -1 or int(nbr.max()) >= n):
        raise ValueError(f'nbr_idx: an index outside -1 .. {n - 1}')
    return nbr.astype(np.int64)


def _nbr_device(nbr_idx, n, dev):
    import torch
    nbr = torch.as_tensor(nbr_idx).to(dev)
    if nbr.dim() != 2 or nbr.is_floating_point() or nbr.dtype == torch.bool or nbr.size(0) != n or nbr.size(1) < 1:
        raise ValueError(f'nbr_idx: an integer tensor [{n}, k], k >= 1')
    if nbr.size(1) > MAX_LISTED:
        raise ValueError(f'nbr_idx: at most {MAX_LISTED} entries per point on the device')
    if nbr.dtype != torch.int32:
        nbr = (nbr.clamp(-2, 2**31 - 1) if nbr.element_size() > 4 else nbr).to(torch.int32)
    return nbr.contiguous()


def _min_neighbours(m):
    if int(m) != m or int(m) < 0:
        raise ValueError(f'min_neighbours {m!r}: an integer >= 0')
    return int(m)


def _normals_f64(xyz, nbr, min_neighbours, return_eigenvalues=False):
    """the twin before the float32 cast -> (normals float64 [n, 3], curvature float64 [n]); with
    ``return_eigenvalues`` also the ascending eigenvalues of C / trace, float64 [n, 3] (NaN where there is no normal)"""
    n, k = nbr.shape
    p = xyz.astype(np.float64)
    valid = nbr >= 0
    safe = np.where(valid, nbr, 0)
    s = p.copy()
    for m in range(k):                                      # list order; an invalid entry adds an exact 0
        s += np.where(valid[:, m, None], p[safe[:, m]], 0.0)
    cnt = valid.sum(1)
    mean = s / (cnt + 1).astype(np.float64)[:, None]
    cov = np.zeros((n, 6), np.float64)
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))

    def add(d, mask):
        for c, (a, b) in enumerate(pairs):
            cov[:, c] += np.where(mask, d[:, a] * d[:, b], 0.0)

    add(p - mean, np.ones(n, bool))
    for m in range(k):
        add(p[safe[:, m]] - mean, valid[:, m])
    tr = (cov[:, 0] + cov[:, 3]) + cov[:, 5]
    with np.errstate(invalid='ignore'):
        has = (cnt >= min_neighbours) & (tr > 0.0) & (tr < np.inf)
    normals = np.zeros((n, 3), np.float64)
    curv = np.zeros(n, np.float64)
    eig = np.full((n, 3), np.nan)
    if has.any():
        c = cov[has] / tr[has, None]
        mat = np.empty((c.shape[0], 3, 3), np.float64)
        mat[:, 0, 0], mat[:, 0, 1], mat[:, 0, 2] = c[:, 0], c[:, 1], c[:, 2]
        mat[:, 1, 0], mat[:, 1, 1], mat[:, 1, 2] = c[:, 1], c[:, 3], c[:, 4]
        mat[:, 2, 0], mat[:, 2, 1], mat[:, 2, 2] = c[:, 2], c[:, 4], c[:, 5]
        lam, vec = np.linalg.eigh(mat)
        v = vec[:, :, 0]
        v = v / np.sqrt((v * v).sum(1))[:, None]
        lead = np.abs(v).argmax(1)                          # (the first of equal magnitudes: the lowest axis)
        v = np.where((v[np.arange(v.shape[0]), lead] < 0.0)[:, None], -v, v)
        normals[has] = v
        total = lam.sum(1)
        l0 = np.maximum(lam[:, 0], 0.0)
        curv[has] = np.where(total > 0.0, l0 / np.where(total > 0.0, total, 1.0), 0.0)
        eig[has] = lam
    return (normals, curv, eig) if return_eigenvalues else (normals, curv)


def point_normals_numpy(xyz, nbr_idx, min_neighbours=3):
    """The definition (``np.linalg.eigh`` in float64) -> (normals float32 [n, 3], curvature float32 [n])"""
    xyz = _xyz_numpy(xyz)
    nbr = _nbr_numpy(nbr_idx, xyz.shape[0])
    normals, curv = _normals_f64(xyz, nbr, _min_neighbours(min_neighbours))
    return normals.astype(np.float32), curv.astype(np.float32)


def _normals_device(xyz, nbr_idx, min_neighbours):
    import torch

    from .. import _lib as L
    xyz = _xyz_device(xyz)
    n, dev = xyz.size(0), xyz.device
    nbr = _nbr_device(nbr_idx, n, dev)
    with torch.cuda.device(dev):
        normals = torch.empty((n, 3), dtype=torch.float32, device=dev)
        curv = torch.empty(n, dtype=torch.float32, device=dev)
        meta = torch.empty(4, dtype=torch.int32, device=dev)
        L.check(L.lib().sg_point_normals(L.ptr(xyz) if n else None, n, L.ptr(nbr) if n else None, nbr.size(1),
                                         min_neighbours, L.ptr(normals) if n else None, L.ptr(curv) if n else None,
                                         L.ptr(meta), L.stream()), 'sg_point_normals')
        if int(meta[1].item()) & _FLAG_INDEX:
            raise ValueError(f'nbr_idx: an index outside -1 .. {n - 1}')
    return normals, curv


def point_normals(xyz, nbr_idx, min_neighbours=3, backend='auto'):
    """``sg_point_normals`` -> (normals float32 [n, 3], curvature float32 [n]) from the neighbour lists ``nbr_idx``
    [n, k] (``knn``'s idx; -1 = no entry).  One read-back (the flags).  An index outside ``-1 .. n - 1`` raises
    ``ValueError``; the device never dereferences one."""
    m = _min_neighbours(min_neighbours)
    if _is_cuda(xyz):
        auto_backend(backend, 'normals')
        return _normals_device(xyz, nbr_idx, m)
    if auto_backend(backend, 'normals') == 'device':
        xyz = _xyz_numpy(xyz)
        _nbr_numpy(nbr_idx, xyz.shape[0])
        return tuple(o.cpu().numpy() for o in _normals_device(_upload(xyz), _upload(_host(nbr_idx)), m))
    return point_normals_numpy(xyz, nbr_idx, m)


# ---- growth ------------------------------------------------------------------------------------------------------------
_SMALL = {'drop': 0, 'absorb': 1}


def _grow_args(angle, max_curvature, max_dist, min_size, small, have_curv, have_d2):
    angle = float(angle)
    if not 0.0 <= angle <= 90.0:
        raise ValueError(f'angle {angle!r}: degrees in [0, 90]')
    if small not in _SMALL:
        raise ValueError(f"small {small!r}: one of 'drop', 'absorb'")
    if int(min_size) != min_size or int(min_size) < 1:
        raise ValueError(f'min_size {min_size!r}: an integer >= 1')
    if max_curvature is not None:
        max_curvature = float(np.float32(max_curvature))
        if max_curvature != max_curvature:
            raise ValueError('max_curvature: None or a number')
        if not have_curv:
            raise ValueError('max_curvature needs curvature')
    md = _max_dist(max_dist)
    if md >= 0.0 and not have_d2:
        raise ValueError('max_dist needs nbr_d2')
    return math.cos(math.radians(angle)), max_curvature, md, int(min_size), _SMALL[small]


def grow_segments_numpy(nbr_idx, normals, curvature=None, nbr_d2=None, angle=10.0, max_curvature=None, max_dist=None,
                        min_size=20, small='absorb'):
    """The definition: the links as an edge list, components by min-label propagation with pointer jumping
    -> (sp int32 [n], n_seg)"""
    cos_thr, mc, md, min_size, absorb = _grow_args(angle, max_curvature, max_dist, min_size, small,
                                                   curvature is not None, nbr_d2 is not None)
    normals = np.ascontiguousarray(_host(normals), dtype=np.float32)
    if normals.ndim != 2 or normals.shape[1] != 3:
        raise ValueError('normals: an array [n, 3]')
    n = normals.shape[0]
    nbr = _nbr_numpy(nbr_idx, n)
    k = nbr.shape[1]
    if n == 0:
        return np.zeros(0, np.int32), 0
    with np.errstate(invalid='ignore'):
        ok = (normals != 0).any(1)
        if mc is not None:
            curv = np.ascontiguousarray(_host(curvature), dtype=np.float32).reshape(n)
            ok &= curv <= np.float32(mc)
        src = np.repeat(np.arange(n), k)
        dst = nbr.reshape(-1)
        keep = (dst >= 0) & (dst != src)
        if md >= 0.0:
            d2 = np.ascontiguousarray(_host(nbr_d2), dtype=np.float64).reshape(n, k)
            keep &= d2.reshape(-1) <= md * md
        src, dst = src[keep], dst[keep]
        keep = ok[src] & ok[dst]
        src, dst = src[keep], dst[keep]
        a, b = normals[src].astype(np.float64), normals[dst].astype(np.float64)
        dot = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
        keep = np.abs(dot) >= cos_thr
    src, dst = src[keep], dst[keep]
    label = np.arange(n)
    # hook and shortcut: label[i] <= i is a forest whose roots are representatives; a round hooks every
    # representative under the smallest representative an edge shows it, then pointer jumping flattens the forest
    for _ in range(n + 1):
        ls, ld = label[src], label[dst]
        low = np.minimum(ls, ld)
        new = label.copy()
        np.minimum.at(new, ls, low)
        np.minimum.at(new, ld, low)
        for _ in range(64):                                 # (a jump halves every path: 2**64 > any path)
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, label):
            break
        label = new
    size = np.bincount(label, minlength=n)
    is_root = (label == np.arange(n)) & (size >= min_size)
    number = np.cumsum(is_root) - 1
    sp = np.where(is_root[label], number[label], -1)
    if absorb:
        listed = np.where(nbr >= 0, sp[np.maximum(nbr, 0)], -1)          # labels from before the pass
        hit = listed >= 0
        first = hit.argmax(1)
        take = (sp < 0) & hit.any(1)
        sp = np.where(take, listed[np.arange(n), first], sp)
    return sp.astype(np.int32), int(is_root.sum())


def _grow_device(nbr_idx, normals, curvature, nbr_d2, cos_thr, mc, md, min_size, absorb):
    import torch

    from .. import _lib as L
    if normals.dim() != 2 or normals.size(1) != 3:
        raise ValueError('normals: a tensor [n, 3]')
    dev = normals.device
    normals = normals.detach().to(torch.float32).contiguous()
    n = normals.size(0)
    if n >= 2**31:
        raise ValueError('normals: fewer than 2**31 points')
    nbr = _nbr_device(nbr_idx, n, dev)
    k = nbr.size(1)
    curv = None
    if mc is not None:
        curv = torch.as_tensor(curvature).to(dev, torch.float32).reshape(-1).contiguous()
        if curv.numel() != n:
            raise ValueError(f'curvature: [{n}]')
    d2 = None
    if md >= 0.0:
        d2 = torch.as_tensor(nbr_d2).to(dev, torch.float64).contiguous()
        if tuple(d2.shape) != (n, k):
            raise ValueError(f'nbr_d2: [{n}, {k}]')
    lib = L.lib()
    with torch.cuda.device(dev):
        sp = torch.empty(n, dtype=torch.int32, device=dev)
        meta = torch.empty(4, dtype=torch.int32, device=dev)
        ws = L.workspace(lib.sg_grow_segments_workspace_bytes(n), dev)
        some = n > 0
        L.check(lib.sg_grow_segments(L.ptr(nbr) if some else None, L.ptr(d2) if (some and d2 is not None) else None, n,
                                     k, L.ptr(normals) if some else None,
                                     L.ptr(curv) if (some and curv is not None) else None, cos_thr,
                                     mc if mc is not None else 0.0, md, min_size, absorb, L.ptr(sp) if some else None,
                                     L.ptr(meta), L.ptr(ws), ws.numel(), L.stream()), 'sg_grow_segments')
        n_seg, flags = meta[:2].cpu().tolist()
    if flags & _FLAG_INDEX:
        raise ValueError(f'nbr_idx: an index outside -1 .. {n - 1}')
    if flags:
        raise L.SoftGroupHipError('grow_segments: a bound of the union-find was hit')
    return sp, n_seg


def grow_segments(nbr_idx, normals, curvature=None, nbr_d2=None, angle=10.0, max_curvature=None, max_dist=None,
                  min_size=20, small='absorb', backend='auto'):
    """``sg_grow_segments`` -> (sp int32 [n], n_seg): the connected components of the links (see the module text);
    ``sp`` is valid input for ``superpoint_index``.  One read-back (``n_seg`` and the flags)."""
    cos_thr, mc, md, min_size, absorb = _grow_args(angle, max_curvature, max_dist, min_size, small,
                                                   curvature is not None, nbr_d2 is not None)
    if _is_cuda(normals):
        auto_backend(backend, 'grow')
        return _grow_device(nbr_idx, normals, curvature, nbr_d2, cos_thr, mc, md, min_size, absorb)
    if auto_backend(backend, 'grow') == 'device':
        normals = np.ascontiguousarray(_host(normals), dtype=np.float32)
        if normals.ndim != 2 or normals.shape[1] != 3:
            raise ValueError('normals: an array [n, 3]')
        _nbr_numpy(nbr_idx, normals.shape[0])
        sp, n_seg = _grow_device(_upload(_host(nbr_idx)), _upload(normals),
                                 None if curvature is None else _upload(_host(curvature)),
                                 None if nbr_d2 is None else _upload(_host(nbr_d2)), cos_thr, mc, md, min_size, absorb)
        return sp.cpu().numpy(), n_seg
    return grow_segments_numpy(nbr_idx, normals, curvature, nbr_d2, angle, max_curvature, max_dist, min_size, small)
