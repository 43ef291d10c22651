"""Instance masks cut into their spatially connected components (``sg_mask_split_count`` / ``_fill``,
csrc/mask_split.hip).

The reference has no such step: nothing in its ``get_instances`` looks at geometry, so one predicted mask may be
a chair plus stray points on the wall behind it, or two chairs welded into one proposal.  The rules are this
project's and are stated in include/softgroup_hip.h; ``mask_components_numpy`` is the definition:

* inside ONE mask, points p != q are adjacent when ``(dx*dx + dy*dy) + dz*dz <= radius*radius`` with
  ``dx = float64(x_p) - float64(x_q)`` -- inclusive, in IEEE double; equal coordinates are adjacent; a point of
  two masks is a node of its own in each;
* a component's key is its smallest point index, its size its number of points;
* ``'split'``: every component with ``size >= min_npoint`` is an output; ``'largest'``: per mask the component of
  greatest size (the smaller key among equal sizes), if it reaches ``min_npoint``;
* outputs in ascending (source mask, key) order: bit row, ``source`` (index of the input mask), ``npoint``;
* a coordinate of a mask point that is not finite, or whose cell ``floor(float64(x) / radius)`` reaches 2**31 in
  magnitude, raises ``ValueError``; points in no mask are never looked at.

Bit rows: integer [n, ceil(N / 32)] of 32-bit words, point i = bit i % 32 of word i / 32; bits at and beyond N
are ignored.  CUDA tensors take the HIP kernels (one read-back, of ``meta``, between the two passes; the count
pass itself reads the number of mask points back once to size its tables); CPU tensors and numpy arrays take
``mask_components_numpy``.
"""
import numpy as np

__all__ = ['mask_components', 'mask_components_numpy', 'split_params', 'MAX_INSTANCES']

MAX_INSTANCES = 16384
_MODE = {'split': 0, 'largest': 1}        # softgroup_hip.h: SG_SPLIT_ALL, SG_SPLIT_LARGEST
_FLAG_NOT_FINITE, _FLAG_CELL_RANGE, _FLAG_INTERNAL, _FLAG_TOO_MANY = 1, 2, 4, 8
_ERR_WORKSPACE = -2
_CELL_LIMIT = 2147483648.0
_GUARD = 2.0 ** -40                       # csrc/mask_split.hip: kMsGuard
_CHUNK = 1 << 22                          # candidate pairs examined at a time (numpy)


def _args(radius, min_npoint, mode):
    if mode not in _MODE:
        raise ValueError(f"mode {mode!r}: one of 'split', 'largest'")
    radius = float(radius)
    if not (radius > 0.0 and np.isfinite(radius) and np.isfinite(radius * radius)):
        raise ValueError(f'radius {radius!r}: a finite number > 0 (with a finite square)')
    if int(min_npoint) != min_npoint or int(min_npoint) < 1:
        raise ValueError(f'min_npoint {min_npoint!r}: an integer >= 1')
    return radius, int(min_npoint), mode


def split_params(split):
    """(radius, min_npoint, mode) of a ``test_cfg.split`` entry (dict or attribute object), validated"""
    get = split.get if isinstance(split, dict) else (lambda k, d=None: getattr(split, k, d))
    radius = get('radius', None)
    if radius is None:
        raise ValueError('test_cfg.split: radius is required')
    return _args(radius, get('min_npoint', 1), get('mode', 'split'))


def _raise_flags(flags):
    if flags & _FLAG_NOT_FINITE:
        raise ValueError('mask_components: a coordinate of a mask point is not finite')
    if flags & _FLAG_CELL_RANGE:
        raise ValueError('mask_components: a mask point whose cell floor(x / radius) reaches 2**31 in magnitude')


def _lookup(table, values):
    """positions of ``values`` in the sorted unique ``table`` and whether they are there"""
    pos = np.minimum(np.searchsorted(table, values), table.size - 1)
    return pos, table[pos] == values


def _edges_numpy(xyz, k_idx, p_idx, radius):
    """(i, j), j < i: the pairs of ids inside one mask within the radius -- cells of ``radius`` keyed by (mask,
    cell), candidates from the 27 offsets (and from the cell beyond where a quotient lies within rounding of a
    cell face: the range ``floor(y - 1 - g) .. floor(y + 1 + g)`` of csrc/mask_split.hip)"""
    P = p_idx.size
    pts = xyz[p_idx].astype(np.float64)
    y = pts / radius
    cell = np.floor(y).astype(np.int64)
    g = _GUARD * np.maximum(1.0, np.abs(y))
    lo = np.maximum(np.floor(y - 1.0 - g), -2147483647.0).astype(np.int64)
    hi = np.minimum(np.floor(y + 1.0 + g), 2147483647.0).astype(np.int64)
    hi = np.minimum(hi, lo + 3)
    lo_off, hi_off = lo - cell, hi - cell
    # (mask, cx) and (cy, cz) compressed separately: no product of ranks leaves int64
    ux, uy, uz = (np.unique(cell[:, d]) for d in range(3))
    rx, ry, rz = (np.searchsorted(u, cell[:, d]) for d, u in enumerate((ux, uy, uz)))
    ua, ia = np.unique(k_idx.astype(np.int64) * ux.size + rx, return_inverse=True)
    ub, ib = np.unique(ry.astype(np.int64) * uz.size + rz, return_inverse=True)
    key = ia.reshape(-1).astype(np.int64) * ub.size + ib.reshape(-1)
    order = np.argsort(key, kind='stable')                  # pairs cell after cell, ids ascending inside a cell
    ukey, gstart, gcount = np.unique(key[order], return_index=True, return_counts=True)
    r2 = radius * radius
    out_i, out_j = [], []
    offs = range(-2, 3)
    side_a = {}
    for dx in offs:
        px, okx = _lookup(ux, cell[:, 0] + dx)
        pa, oka = _lookup(ua, k_idx.astype(np.int64) * ux.size + px)
        side_a[dx] = (pa, okx & oka & (lo_off[:, 0] <= dx) & (dx <= hi_off[:, 0]))
    for dy in offs:
        py, oky = _lookup(uy, cell[:, 1] + dy)
        oky &= (lo_off[:, 1] <= dy) & (dy <= hi_off[:, 1])
        if not oky.any():
            continue
        for dz in offs:
            pz, okz = _lookup(uz, cell[:, 2] + dz)
            pb, okb = _lookup(ub, py.astype(np.int64) * uz.size + pz)
            okb &= oky & okz & (lo_off[:, 2] <= dz) & (dz <= hi_off[:, 2])
            if not okb.any():
                continue
            for dx in offs:
                pa, oka = side_a[dx]
                ok = oka & okb
                src = np.flatnonzero(ok)
                if src.size == 0:
                    continue
                grp, found = _lookup(ukey, pa[src] * ub.size + pb[src])
                src, grp = src[found], grp[found]
                cnt = gcount[grp]
                # candidates in chunks: pair src[t] against the members of its neighbour cell
                ends = np.cumsum(cnt)
                t0 = 0
                while t0 < src.size:
                    base = ends[t0 - 1] if t0 else 0
                    t1 = max(int(np.searchsorted(ends, base + _CHUNK, side='right')), t0 + 1)
                    c = cnt[t0:t1]
                    total = int(c.sum())
                    rep = np.repeat(np.arange(t0, t1), c)
                    within = np.arange(total) - np.repeat(ends[t0:t1] - c - base, c)
                    i = src[rep]
                    j = order[gstart[grp[rep]] + within]
                    lower = j < i
                    i, j = i[lower], j[lower]
                    d = pts[i] - pts[j]
                    near = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= r2
                    out_i.append(i[near])
                    out_j.append(j[near])
                    t0 = t1
    if not out_i:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(out_i), np.concatenate(out_j)


def _labels_numpy(P, ei, ej):
    """root of every id: min-label propagation with pointer jumping until nothing changes; lab[i] <= i throughout,
    so a root is the smallest id of its tree"""
    lab = np.arange(P, dtype=np.int64)
    while ei.size:
        a, b = lab[ei], lab[ej]
        differ = a != b
        if not differ.any():
            break
        ei, ej, a, b = ei[differ], ej[differ], a[differ], b[differ]
        np.minimum.at(lab, np.maximum(a, b), np.minimum(a, b))       # the larger root under the smaller
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
    return lab


def mask_components_numpy(bits, n_points, xyz, radius, min_npoint=1, mode='split'):
    """The definition, on the host.  ``bits``: integer rows [n, ceil(N / 32)] of 32-bit words, or their bytes
    (uint8 [n, >= ceil(N / 8)], little-endian bit order); ``xyz`` [N, 3] (cast to float32).
    -> (out_bits int32 [n_out, ceil(N / 32)], source int32 [n_out], npoint int32 [n_out])"""
    radius, min_npoint, mode = _args(radius, min_npoint, mode)
    n_points = int(n_points)
    words = (n_points + 31) // 32
    bits = np.ascontiguousarray(np.asarray(bits))
    if bits.ndim != 2 or bits.dtype.kind not in 'iu':
        raise ValueError(f'bits: integer rows [n, {words}] of 32-bit words')
    n = bits.shape[0]
    rows = bits.view(np.uint8).reshape(n, -1) if n else np.zeros((0, words * 4), np.uint8)
    if n and rows.shape[1] * 8 < n_points:
        raise ValueError(f'bits: rows of {rows.shape[1] * 8} bits for {n_points} points')
    xyz = np.ascontiguousarray(np.asarray(xyz), dtype=np.float32)
    if xyz.ndim != 2 or xyz.shape != (n_points, 3):
        raise ValueError(f'xyz: an array [{n_points}, 3]')
    empty = (np.zeros((0, words), np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    if n == 0 or n_points == 0:
        return empty
    dense = np.unpackbits(rows, axis=1, bitorder='little')[:, :n_points]
    k_idx, p_idx = np.nonzero(dense)                        # ids: ascending (mask, point)
    P = p_idx.size
    if P == 0:
        return empty
    used = xyz[np.flatnonzero(dense.any(0))].astype(np.float64)
    if not np.isfinite(used).all():
        _raise_flags(_FLAG_NOT_FINITE)
    if not (np.abs(np.floor(used / radius)) < _CELL_LIMIT).all():
        _raise_flags(_FLAG_CELL_RANGE)
    ei, ej = _edges_numpy(xyz, k_idx, p_idx, radius)
    lab = _labels_numpy(P, ei, ej)
    roots = np.flatnonzero(lab == np.arange(P))             # ascending id = ascending (mask, key)
    size = np.bincount(lab, minlength=P)[roots]
    if mode == 'largest':
        first = np.lexsort((roots, -size, k_idx[roots]))    # per mask: the greatest size, then the smaller key
        mk = k_idx[roots][first]
        head = np.ones(first.size, bool)
        head[1:] = mk[1:] != mk[:-1]
        keep = np.zeros(roots.size, bool)
        keep[first[head]] = True
        keep &= size >= min_npoint
    else:
        keep = size >= min_npoint
    roots, size = roots[keep], size[keep]
    n_out = roots.size
    outidx = np.full(P, -1, np.int64)
    outidx[roots] = np.arange(n_out)
    row = outidx[lab]
    sel = row >= 0
    out = np.zeros((n_out, words * 32), dtype=bool)
    out[row[sel], p_idx[sel]] = True
    packed = np.packbits(out, axis=1, bitorder='little') if n_out else np.zeros((0, words * 4), np.uint8)
    return (np.ascontiguousarray(packed).view(np.int32).reshape(n_out, words), k_idx[roots].astype(np.int32),
            size.astype(np.int32))


def components_device_raw(bits_ptr, n, n_points, xyz, radius, min_npoint, mode, device):
    """``sg_mask_split_count`` / ``_fill`` on rows at a raw device address (a tensor's, or the scan's arena)
    -> (out_bits int32 [n_out, words], source int32, npoint int32) on ``device``.  One read-back, of ``meta``."""
    import torch

    from .. import _lib as L
    radius, min_npoint, mode = _args(radius, min_npoint, mode)
    lib = L.lib()
    n, n_points = int(n), int(n_points)
    words = (n_points + 31) // 32
    if xyz.dim() != 2 or tuple(xyz.shape) != (n_points, 3):
        raise ValueError(f'xyz: a tensor [{n_points}, 3]')
    xyz = xyz.detach().to(device, torch.float32).contiguous()
    with torch.cuda.device(device):
        # the tables grow with the number of mask points, which only the device knows: a first size for a few
        # masks' worth of the cloud, the exact one when the count pass says it was too small
        guess = min(n * n_points, 4 * n_points + 65536, 2**31 - 1)
        nb = lib.sg_mask_split_workspace_bytes(n, n_points, guess)
        if nb == 0:
            raise L.SoftGroupHipError(f'mask_components: {n} masks over {n_points} points: outside the supported '
                                      f'range (at most {MAX_INSTANCES} masks, fewer than 2**31 points)')
        meta = torch.empty(4, dtype=torch.int32, device=device)
        ws = L.workspace(nb, device)
        args = (L.ptr(xyz) if n_points else None, bits_ptr, n, n_points, radius, min_npoint, _MODE[mode], L.ptr(meta))
        rc = lib.sg_mask_split_count(*args, L.ptr(ws), ws.numel(), L.stream())
        if rc == _ERR_WORKSPACE:
            nb = lib.sg_mask_split_workspace_bytes(n, n_points, int(meta[2].item()))
            ws = L.workspace(nb, device)
            rc = lib.sg_mask_split_count(*args, L.ptr(ws), ws.numel(), L.stream())
        L.check(rc, 'sg_mask_split_count')
        n_out, flags, n_pairs, _ = meta.cpu().tolist()
        _raise_flags(flags)
        if flags & _FLAG_TOO_MANY:
            raise L.SoftGroupHipError(f'mask_components: {n_out} components survive, at most {MAX_INSTANCES} are '
                                      'supported (raise min_npoint)')
        if flags:
            raise L.SoftGroupHipError(f'sg_mask_split_count: internal bound hit (flags {flags})')
        out_bits = torch.empty((n_out, words), dtype=torch.int32, device=device)
        source = torch.empty(n_out, dtype=torch.int32, device=device)
        npoint = torch.empty(n_out, dtype=torch.int32, device=device)
        if n_out:
            L.check(lib.sg_mask_split_fill(n, n_points, n_pairs, L.ptr(ws), ws.numel(), n_out, L.ptr(out_bits),
                                           L.ptr(source), L.ptr(npoint), L.stream()), 'sg_mask_split_fill')
    return out_bits, source, npoint


def mask_components(bits, n_points, xyz, radius, min_npoint=1, mode='split'):
    """-> (out_bits int32 [n_out, ceil(N / 32)], source int32 [n_out], npoint int32 [n_out]) where ``bits``
    lives.  CUDA bits: the HIP kernels (``xyz`` is brought to that device), device tensors.  CPU tensors and numpy
    arrays: ``mask_components_numpy`` (tensors in, tensors out)."""
    import torch
    radius, min_npoint, mode = _args(radius, min_npoint, mode)
    n_points = int(n_points)
    words = (n_points + 31) // 32
    if not torch.is_tensor(bits):
        return mask_components_numpy(bits, n_points, xyz.detach().cpu().numpy() if torch.is_tensor(xyz) else xyz,
                                     radius, min_npoint, mode)
    if bits.dim() != 2 or bits.element_size() != 4 or bits.is_floating_point() or bits.size(1) != words:
        raise ValueError(f'bits: an integer tensor [n, {words}] of 32-bit words')
    if not bits.is_cuda:
        h_xyz = xyz.detach().cpu().numpy() if torch.is_tensor(xyz) else xyz
        out = mask_components_numpy(bits.contiguous().numpy(), n_points, h_xyz, radius, min_npoint, mode)
        return tuple(torch.from_numpy(o) for o in out)
    bits = bits.contiguous()
    xyz = torch.as_tensor(xyz)
    return components_device_raw(bits.data_ptr() if bits.numel() else None, bits.size(0), n_points, xyz, radius,
                                 min_npoint, mode, bits.device)
