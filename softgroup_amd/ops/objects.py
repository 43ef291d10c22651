"""The object table of a mask list (csrc/objects.hip): per mask its population, axis-aligned box, centroid, centred
second moments and colour mean (``instance_moments``), its extents along a table of yaw directions and the direction
of the smallest enclosing rectangle (``instance_extents``), and its semantic vote (``instance_class_hist``).

The reference has none of these; the rules are this project's and are stated in include/softgroup_hip.h:

inputs
  ``bits`` integer [n, ceil(N / 32)]: point i is bit ``i % 32`` of word ``i / 32``, bits at and beyond N are ignored;
  ``coords`` float32 [N, 3]; ``colors`` float32 [N, 3], optional; ``semantic`` int32 or int64 [N], optional, with
  ``n_classes`` in 1 .. 256.  Device range: up to 16 384 masks and fewer than 2**31 points.  A point of at least one
  mask whose coordinate (or colour, when given) is not finite sets the flag that ``describe_instances`` turns into
  ``ValueError`` on both backends; a non-finite value at a point that is in no mask is never an error.
1. population and box
  ``npoint[m]`` the number of mask points; ``aabb[m] = (xmin, ymin, zmin, xmax, ymax, zmax)`` in float64 from the
  float32 coordinates.  EVERY extreme of this stage is canonicalised with ``+ 0.0`` (``-0.0`` becomes ``+0.0``:
  ``np.min`` over ``{-0.0, +0.0}`` depends on the order).
2. sums in a fixed order
  a sum over the points of mask m of a double ``v(i)``: LEAF of word w: ``acc = +0.0``, then ``acc = acc +
  v(32 w + b)`` for the set bits b in ascending order; TREE: the leaves of words ``0 .. W-1``, padded with ``+0.0``
  to the next power of two, are added in adjacent pairs ``a'[k] = a[2k] + a[2k+1]``, level by level (a leaf is never
  ``-0.0``, so skipping an all-zero subtree is exact).  ``sum_xyz[m]`` = the sums of ``double(x)``, ``double(y)``,
  ``double(z)``; ``centroid = sum / double(npoint)``, one division each; ``cov6[m]`` = the six sums ``(dx dx, dx dy,
  dx dz, dy dy, dy dz, dz dz)`` with ``dx = double(x) - cx``, each product one multiplication, each sum divided once
  by ``double(npoint)``; ``mean_color[m]`` = the three colour sums divided by ``double(npoint)``.  No float atomics.
3. yaw sweep
  ``yaw_steps = A`` in 1 .. 180, ``theta_a = a * (pi / 2) / A``; ``c_a = np.cos(theta_a)``, ``s_a = np.sin(theta_a)``
  once on the host in float64, one table [A, 2] for both backends (``yaw_table``).  Per mask point ``u = double(x) *
  c + double(y) * s`` and ``v = double(y) * c - double(x) * s`` (two products and one add or subtract each, no
  contraction; elementwise numpy in the twin).  Per (mask, angle) ``umin, umax, vmin, vmax``, each ``+ 0.0``; ``area
  = (umax - umin) * (vmax - vmin)``; the chosen angle is the one of smallest area, the lowest index among equal areas.
4. refinement
  ``refine = r`` in 0 .. 8: a second sweep per mask over the ``2 r + 1`` angles ``theta_best + j * step / (r + 1)``,
  j = -r .. r, ``step = (pi / 2) / A``; per-mask tables [n, 2 r + 1, 2] from the host (``refine_tables``: a table per
  coarse winner, gathered by the winner's index), hence the row stride of the sweep (0: one shared table).  j = 0 is
  the coarse winner, so the refined area is never larger.
5. box composition (``compose_boxes``, host code for both backends)
  ``uc = (umin + umax) * 0.5``, ``vc`` likewise; ``cx = uc * c - vc * s``, ``cy = uc * s + vc * c``, ``cz = (zmin +
  zmax) * 0.5``; ``obb[m] = (cx, cy, cz, du, dv, dz, theta)``, ``du = umax - umin`` along ``(cos theta, sin theta)``,
  ``dv`` along ``(-sin theta, cos theta)``; ``theta`` as computed, not wrapped.
6. semantic vote
  per mask a histogram of the labels in ``0 .. n_classes-1`` over its points (other values are not counted);
  ``sem_label[m]`` the class of the greatest count, the lowest among equal counts, ``sem_count[m]`` that count (purity
  = ``sem_count / npoint``); ``-1 / 0`` for a mask without a counted label.  Integer atomics only.
7. empty masks
  ``npoint`` 0, every float output NaN, the angle index -1, ``sem_label`` -1.

CUDA tensors take the HIP kernels (nothing synchronises; the flags come back as a tensor), numpy arrays the
``*_numpy`` twins on the packed rows, which are the definition the device results are held to byte for byte.
"""
import numpy as np

from ._args import _words, choose_backend

__all__ = ['auto_backend', 'yaw_table', 'refine_tables', 'compose_boxes', 'instance_moments', 'instance_moments_numpy',
           'instance_extents', 'instance_extents_numpy', 'instance_class_hist', 'instance_class_hist_numpy',
           'MAX_INSTANCES', 'MAX_CLASSES', 'MAX_YAW_STEPS', 'MAX_REFINE', 'MAX_DEVICE_POINTS', 'FLAG_NOT_FINITE']

MAX_INSTANCES = 16384
MAX_CLASSES = 256
MAX_YAW_STEPS = 180
MAX_REFINE = 8
MAX_DEVICE_POINTS = 2**31
FLAG_NOT_FINITE = 1

# what backend='auto' means with a GPU present -- the single place to change.  It follows profiles/objects_bench.txt,
# where ``describe_instances`` on the device is ahead of the numpy twins on every measured list by far more than the
# spread of the five repetitions (wall, MI355X, numpy arrays and RLE dicts in, the table out): 1.1 / 1.4 / 3.3 ms
# against 462 / 1353 / 5254 ms.
_AUTO = {'describe': 'device'}


def auto_backend(backend, what='describe'):
    """'device' or 'numpy' for one of the operations of ``_AUTO``"""
    return choose_backend(backend, _AUTO[what])


# ---- host tables and box composition (shared by both backends) ---------------------------------------------------------
def _yaw_steps(yaw_steps):
    if isinstance(yaw_steps, bool) or int(yaw_steps) != yaw_steps or not 1 <= int(yaw_steps) <= MAX_YAW_STEPS:
        raise ValueError(f'yaw_steps {yaw_steps!r}: an integer between 1 and {MAX_YAW_STEPS}')
    return int(yaw_steps)


def _refine(refine):
    if isinstance(refine, bool) or int(refine) != refine or not 0 <= int(refine) <= MAX_REFINE:
        raise ValueError(f'refine {refine!r}: an integer between 0 and {MAX_REFINE}')
    return int(refine)


def _cos_sin(theta):
    return np.stack([np.cos(theta), np.sin(theta)], axis=-1)


def yaw_table(yaw_steps):
    """-> (theta float64 [A], table float64 [A, 2] of (cos, sin)): ``theta_a = a * (pi / 2) / A``"""
    a = _yaw_steps(yaw_steps)
    theta = np.arange(a, dtype=np.float64) * (np.pi / 2) / np.float64(a)
    return theta, _cos_sin(theta)


def refine_tables(yaw_steps, refine):
    """-> (theta float64 [A, 2 r + 1], tables float64 [A, 2 r + 1, 2]): row a holds the angles ``theta_a + j * step /
    (r + 1)``, j = -r .. r, of a mask whose coarse winner is a"""
    a, r = _yaw_steps(yaw_steps), _refine(refine)
    theta, _ = yaw_table(a)
    step = (np.pi / 2) / np.float64(a)
    j = np.arange(-r, r + 1, dtype=np.float64)
    fine = theta[:, None] + j[None, :] * step / np.float64(r + 1)
    return fine, _cos_sin(fine)


def compose_boxes(ext, cs, theta, zmin, zmax):
    """ext float64 [n, 4] = (umin, umax, vmin, vmax) of the chosen angle, cs [n, 2] its (cos, sin), theta [n], zmin /
    zmax [n] -> obb float64 [n, 7] = (cx, cy, cz, du, dv, dz, theta)"""
    ext, cs = np.asarray(ext, np.float64).reshape(-1, 4), np.asarray(cs, np.float64).reshape(-1, 2)
    theta, zmin, zmax = (np.asarray(v, np.float64).reshape(-1) for v in (theta, zmin, zmax))
    umin, umax, vmin, vmax = ext[:, 0], ext[:, 1], ext[:, 2], ext[:, 3]
    c, s = cs[:, 0], cs[:, 1]
    uc, vc = (umin + umax) * 0.5, (vmin + vmax) * 0.5
    return np.stack([uc * c - vc * s, uc * s + vc * c, (zmin + zmax) * 0.5, umax - umin, vmax - vmin, zmax - zmin,
                     theta], axis=1)


# ---- the twins -------------------------------------------------------------------------------------------------------
def _rows32(bits, n_points):
    """packed rows of any integer dtype -> uint32 [n, ceil(n_points / 32)], bits at and beyond n_points cleared"""
    bits = np.ascontiguousarray(bits)
    if bits.ndim != 2 or bits.dtype.kind not in 'iu':
        raise ValueError('bits: an integer array [n, ceil(n_points / 32)] of packed rows')
    n, words = bits.shape[0], _words(n_points)
    if bits.shape[1] * bits.dtype.itemsize != words * 4:
        raise ValueError(f'bits: rows of {bits.shape[1] * bits.dtype.itemsize} bytes for {n_points} points '
                         f'({words * 4} bytes)')
    rows = (bits.view(np.uint32).reshape(n, words) if n and words else np.zeros((n, words), np.uint32)).copy()
    if words and n_points & 31:
        rows[:, -1] &= np.uint32((1 << (n_points & 31)) - 1)
    return rows


def _points_numpy(a, n_points, what):
    a = np.ascontiguousarray(np.asarray(a), dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] != n_points:
        raise ValueError(f'{what}: an array [{n_points}, 3], one row per point of the masks')
    return a


_BITS = np.arange(32, dtype=np.uint32)
_BLOCK = 1 << 15                                             # (mask, word) pairs per vectorised step of the twins


def _pairs(rows):
    """rows uint32 [n, W] -> the non-zero (mask, word) pairs in (mask, word) order"""
    mz, wz = np.nonzero(rows)
    return mz.astype(np.int64), wz.astype(np.int64), rows[mz, wz]


def _member(word):
    return ((word[:, None] >> _BITS[None, :]) & np.uint32(1)).astype(bool)


def _mask_points(rows):
    """-> (the mask of every (mask, point) pair, its point), in (mask, point) order; the population of every mask"""
    mz, wz, word = _pairs(rows)
    owner, point = [], []
    for lo in range(0, mz.size, _BLOCK):
        member = _member(word[lo:lo + _BLOCK])
        k, b = np.nonzero(member)
        owner.append(mz[lo:lo + _BLOCK][k]), point.append(wz[lo:lo + _BLOCK][k] * 32 + b)
    owner = np.concatenate(owner) if owner else np.zeros(0, np.int64)
    point = np.concatenate(point) if point else np.zeros(0, np.int64)
    return owner, point, np.bincount(owner, minlength=rows.shape[0]).astype(np.int64)


def _ordered_sums(rows, value_of):
    """The fixed-order sums of every mask: ``value_of(mask ids [K], point ids [32, K]) -> float64 [32, K, Q]`` gives
    the values at the 32 points of K (mask, word) pairs.  LEAF: 32 sequential additions per word (a point outside
    the mask adds +0.0).  TREE: level by level, the entries (mask, word) whose words are 2k and 2k + 1 become
    (mask, k) with the sum of the two; a word without a partner is padded with +0.0, which leaves it as it is (a
    partial is never -0.0).  -> float64 [n, Q], +0.0 for an empty mask"""
    n, words = rows.shape
    mz, wz, word = _pairs(rows)
    leaves = []
    for lo in range(0, mz.size, _BLOCK):
        member = _member(word[lo:lo + _BLOCK]).T                                # [32, K]
        idx = wz[None, lo:lo + _BLOCK] * 32 + np.arange(32)[:, None]
        v = np.where(member[:, :, None], value_of(mz[lo:lo + _BLOCK], idx), 0.0)
        acc = np.zeros(v.shape[1:], np.float64)
        for b in range(32):
            acc = acc + v[b]
        leaves.append(acc)
    if not leaves:
        return None
    v = np.concatenate(leaves)
    size = 1
    while size < words:
        size *= 2
        parent = wz >> 1
        first = np.ones(mz.size, bool)
        first[1:] = (mz[1:] != mz[:-1]) | (parent[1:] != parent[:-1])
        left, right = np.flatnonzero(first), np.flatnonzero(~first)        # (a right entry follows its left one)
        out = v[left]
        at = np.searchsorted(left, right - 1)
        out[at] = out[at] + v[right]
        mz, wz, v = mz[left], parent[left], out
    total = np.zeros((n, v.shape[1]), np.float64)
    total[mz] = v
    return total


def instance_moments_numpy(bits, n_points, coords, colors=None):
    """packed rows [n, ceil(n_points / 32)], coords float32 [n_points, 3], colors float32 [n_points, 3] or None -> a
    dict of ``npoint`` int32 [n], ``aabb`` [n, 6], ``sum_xyz`` [n, 3], ``centroid`` [n, 3], ``cov6`` [n, 6] float64,
    with colours ``mean_color`` [n, 3], and ``flags`` (int)"""
    n_points = int(n_points)
    rows = _rows32(bits, n_points)
    n, words = rows.shape
    xyz = np.zeros((words * 32, 3), np.float64)
    xyz[:n_points] = _points_numpy(coords, n_points, 'coords')
    rgb = None
    if colors is not None:
        rgb = np.zeros((words * 32, 3), np.float64)
        rgb[:n_points] = _points_numpy(colors, n_points, 'colors')
    out = {'npoint': np.zeros(n, np.int32), 'aabb': np.full((n, 6), np.nan), 'sum_xyz': np.full((n, 3), np.nan),
           'centroid': np.full((n, 3), np.nan), 'cov6': np.full((n, 6), np.nan)}
    if rgb is not None:
        out['mean_color'] = np.full((n, 3), np.nan)
    out['flags'] = 0
    owner, point, npoint = _mask_points(rows)
    some = npoint > 0
    if not some.any():
        return out
    with np.errstate(all='ignore'):
        own = xyz[point]
        if not np.isfinite(own).all() or (rgb is not None and not np.isfinite(rgb[point]).all()):
            out['flags'] |= FLAG_NOT_FINITE
        starts = (np.cumsum(npoint) - npoint)[some]
        out['npoint'][:] = npoint
        out['aabb'][some, :3] = np.minimum.reduceat(own, starts, axis=0) + 0.0
        out['aabb'][some, 3:] = np.maximum.reduceat(own, starts, axis=0) + 0.0
        count = npoint[some].astype(np.float64)[:, None]
        sums = _ordered_sums(rows, lambda m, idx: xyz[idx])
        cen = np.full((n, 3), np.nan)
        cen[some] = sums[some] / count
        out['sum_xyz'][some], out['centroid'][some] = sums[some], cen[some]

        def products(m, idx):
            d = xyz[idx] - cen[m][None, :, :]
            dx, dy, dz = d[:, :, 0], d[:, :, 1], d[:, :, 2]
            return np.stack([dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz], axis=2)

        out['cov6'][some] = _ordered_sums(rows, products)[some] / count
        if rgb is not None:
            out['mean_color'][some] = _ordered_sums(rows, lambda m, idx: rgb[idx])[some] / count
    return out


def _table_numpy(table, n, row_stride):
    table = np.ascontiguousarray(np.asarray(table), dtype=np.float64)
    if row_stride:
        if table.ndim != 3 or table.shape[0] != n or table.shape[2] != 2:
            raise ValueError('table: an array [n, A, 2] with a row stride')
        n_ang = table.shape[1]
    else:
        if table.ndim != 2 or table.shape[1] != 2:
            raise ValueError('table: an array [A, 2]')
        n_ang = table.shape[0]
    if not 1 <= n_ang <= MAX_YAW_STEPS or row_stride not in (0, n_ang):
        raise ValueError(f'table: between 1 and {MAX_YAW_STEPS} angles, a row stride of 0 or the angle count')
    return table, n_ang


def instance_extents_numpy(bits, n_points, coords, table, row_stride=0):
    """packed rows, coords, table float64 [A, 2] (``row_stride`` 0) or [n, A, 2] (``row_stride`` A) -> a dict of
    ``best_index`` int32 [n], ``best_ext`` float64 [n, 4] = (umin, umax, vmin, vmax) of the chosen angle, ``all_ext``
    float64 [n, A, 4] and ``flags`` (int).  Elementwise numpy only: no ``dot``."""
    n_points = int(n_points)
    rows = _rows32(bits, n_points)
    n = rows.shape[0]
    table, n_ang = _table_numpy(table, n, int(row_stride))
    xy = np.ascontiguousarray(_points_numpy(coords, n_points, 'coords')[:, :2], dtype=np.float64)
    out = {'best_index': np.full(n, -1, np.int32), 'best_ext': np.full((n, 4), np.nan),
           'all_ext': np.full((n, n_ang, 4), np.nan), 'flags': 0}
    owner, point, npoint = _mask_points(rows)
    some = npoint > 0
    if not some.any():
        return out
    with np.errstate(all='ignore'):
        own = xy[point]
        if not np.isfinite(own).all():
            out['flags'] |= FLAG_NOT_FINITE
        ext = np.empty((n, n_ang, 4), np.float64)
        ext[:, :, 0::2], ext[:, :, 1::2] = np.inf, -np.inf
        step = max(1, (1 << 21) // n_ang)
        for lo in range(0, own.shape[0], step):                     # (extremes are order-free: any split is exact)
            who = owner[lo:lo + step]
            x, y = own[lo:lo + step, 0:1], own[lo:lo + step, 1:2]
            cs = table[who] if row_stride else table[None]
            c, s = cs[:, :, 0], cs[:, :, 1]
            u = x * c + y * s
            v = y * c - x * s
            starts = np.flatnonzero(np.concatenate([[True], who[1:] != who[:-1]]))
            ids = who[starts]
            ext[ids, :, 0] = np.minimum(ext[ids, :, 0], np.minimum.reduceat(u, starts, axis=0))
            ext[ids, :, 1] = np.maximum(ext[ids, :, 1], np.maximum.reduceat(u, starts, axis=0))
            ext[ids, :, 2] = np.minimum(ext[ids, :, 2], np.minimum.reduceat(v, starts, axis=0))
            ext[ids, :, 3] = np.maximum(ext[ids, :, 3], np.maximum.reduceat(v, starts, axis=0))
        ext = ext[some] + 0.0
        area = (ext[:, :, 1] - ext[:, :, 0]) * (ext[:, :, 3] - ext[:, :, 2])
        best, best_area = np.zeros(ext.shape[0], np.int64), area[:, 0]
        for a in range(1, n_ang):                                   # the device's comparisons: strictly smaller wins
            better = area[:, a] < best_area
            best, best_area = np.where(better, a, best), np.where(better, area[:, a], best_area)
        out['all_ext'][some], out['best_index'][some] = ext, best
        out['best_ext'][some] = ext[np.arange(ext.shape[0]), best]
    return out


def _n_classes(n_classes):
    if n_classes is None or isinstance(n_classes, bool) or int(n_classes) != n_classes or int(n_classes) < 1:
        raise ValueError(f'n_classes {n_classes!r}: an integer >= 1')
    return int(n_classes)


def instance_class_hist_numpy(bits, n_points, semantic, n_classes):
    """packed rows, semantic integer [n_points] -> a dict of ``hist`` int32 [n, C], ``sem_label``, ``sem_count`` int32
    [n] (any C >= 1)"""
    n_points, n_cls = int(n_points), _n_classes(n_classes)
    rows = _rows32(bits, n_points)
    n = rows.shape[0]
    semantic = np.asarray(semantic).reshape(-1)
    if semantic.dtype.kind not in 'iu' or semantic.size != n_points:
        raise ValueError(f'semantic: an integer array [{n_points}], one label per point of the masks')
    owner, point, _ = _mask_points(rows)
    lab = semantic.astype(np.int64)[point]
    ok = (lab >= 0) & (lab < n_cls)
    hist = np.bincount(owner[ok] * n_cls + lab[ok], minlength=n * n_cls).astype(np.int32).reshape(n, n_cls)
    count = hist.max(1) if n else np.zeros(0, np.int32)
    label = np.where(count > 0, hist.argmax(1), -1).astype(np.int32) if n else np.zeros(0, np.int32)
    return {'hist': hist, 'sem_label': label, 'sem_count': count.astype(np.int32)}


# ---- the device ------------------------------------------------------------------------------------------------------
def _bit_rows(bits, n_points, who):
    from .. import _lib as L
    if bits.dim() != 2 or bits.element_size() != 4 or bits.is_floating_point() or bits.size(1) != _words(n_points):
        raise ValueError(f'bits: an integer tensor [n, {_words(n_points)}] of 32-bit words')
    if bits.size(0) > MAX_INSTANCES or n_points >= MAX_DEVICE_POINTS:
        raise L.SoftGroupHipError(f'{who}: {bits.size(0)} masks over {n_points} points: outside the supported range '
                                  f'(at most {MAX_INSTANCES}, fewer than 2**31)')
    return bits.contiguous()


def _points_device(a, n_points, what, dev):
    import torch
    if not (torch.is_tensor(a) and a.is_cuda):
        raise ValueError(f'{what}: a CUDA tensor, like bits')
    if a.dim() != 2 or a.size(1) != 3 or a.size(0) != n_points:
        raise ValueError(f'{what}: a tensor [{n_points}, 3], one row per point of the masks')
    return a.detach().to(dev, torch.float32).contiguous()


def instance_moments(bits, n_points, coords, colors=None):
    """``sg_instance_moments`` on CUDA bit rows int32 [n, ceil(n_points / 32)] and CUDA coords (colors) -> the dict of
    ``instance_moments_numpy`` as CUDA tensors, ``flags`` an int32 tensor [1].  Nothing synchronises.  Other inputs:
    numpy."""
    import torch
    if not (torch.is_tensor(bits) and bits.is_cuda):
        return instance_moments_numpy(bits, n_points, coords, colors)
    from .. import _lib as L
    n_points = int(n_points)
    bits = _bit_rows(bits, n_points, 'instance_moments')
    dev, n = bits.device, bits.size(0)
    coords = _points_device(coords, n_points, 'coords', dev)
    colors = None if colors is None else _points_device(colors, n_points, 'colors', dev)
    lib = L.lib()
    with torch.cuda.device(dev):
        f64 = dict(dtype=torch.float64, device=dev)
        out = {'npoint': torch.empty(n, dtype=torch.int32, device=dev), 'aabb': torch.empty((n, 6), **f64),
               'sum_xyz': torch.empty((n, 3), **f64), 'centroid': torch.empty((n, 3), **f64),
               'cov6': torch.empty((n, 6), **f64)}
        if colors is not None:
            out['mean_color'] = torch.empty((n, 3), **f64)
        flags = torch.empty(1, dtype=torch.int32, device=dev)
        ws = L.workspace(lib.sg_instance_moments_workspace_bytes(n, n_points), dev)
        L.check(lib.sg_instance_moments(L.ptr(bits) if bits.numel() else None, n, n_points,
                                        L.ptr(coords) if n_points else None,
                                        L.ptr(colors) if colors is not None and n_points else None,
                                        L.ptr(out['npoint']), L.ptr(out['aabb']), L.ptr(out['sum_xyz']),
                                        L.ptr(out['centroid']), L.ptr(out['cov6']), L.ptr(out.get('mean_color')),
                                        L.ptr(flags), L.ptr(ws), ws.numel(), L.stream()), 'sg_instance_moments')
        if colors is not None and n_points == 0:
            out['mean_color'].fill_(float('nan'))                   # (no colour array was handed on)
    out['flags'] = flags
    return out


def instance_extents(bits, n_points, coords, table, row_stride=0, all_extents=False):
    """``sg_instance_extents`` on CUDA bit rows and coords; ``table`` float64 [A, 2] (``row_stride`` 0) or [n, A, 2]
    (``row_stride`` A), host or device -> a dict of ``best_index`` int32 [n], ``best_ext`` float64 [n, 4], with
    ``all_extents`` also ``all_ext`` float64 [n, A, 4], and ``flags`` int32 [1], on the device.  Nothing
    synchronises.  Other inputs: numpy."""
    import torch
    if not (torch.is_tensor(bits) and bits.is_cuda):
        return instance_extents_numpy(bits, n_points, coords, table.cpu().numpy() if torch.is_tensor(table) else table,
                                      row_stride)
    from .. import _lib as L
    n_points, row_stride = int(n_points), int(row_stride)
    bits = _bit_rows(bits, n_points, 'instance_extents')
    dev, n = bits.device, bits.size(0)
    coords = _points_device(coords, n_points, 'coords', dev)
    table = torch.as_tensor(table).to(dev, torch.float64).contiguous()
    if table.dim() != (3 if row_stride else 2) or table.size(-1) != 2 or (row_stride and table.size(0) != n):
        raise ValueError('table: [A, 2], or [n, A, 2] with a row stride')
    n_ang = table.size(-2)
    if not 1 <= n_ang <= MAX_YAW_STEPS or row_stride not in (0, n_ang):
        raise ValueError(f'table: between 1 and {MAX_YAW_STEPS} angles, a row stride of 0 or the angle count')
    lib = L.lib()
    with torch.cuda.device(dev):
        out = {'best_index': torch.empty(n, dtype=torch.int32, device=dev),
               'best_ext': torch.empty((n, 4), dtype=torch.float64, device=dev)}
        ws = None
        if all_extents:
            out['all_ext'] = torch.empty((n, n_ang, 4), dtype=torch.float64, device=dev)
        else:
            ws = L.workspace(lib.sg_instance_extents_workspace_bytes(n, n_ang), dev)
        flags = torch.empty(1, dtype=torch.int32, device=dev)
        L.check(lib.sg_instance_extents(L.ptr(bits) if bits.numel() else None, n, n_points,
                                        L.ptr(coords) if n_points else None, L.ptr(table), row_stride, n_ang,
                                        L.ptr(out['best_index']), L.ptr(out['best_ext']),
                                        L.ptr(out['all_ext']) if all_extents and n else None, L.ptr(flags),
                                        L.ptr(ws), ws.numel() if ws is not None else 0, L.stream()),
                'sg_instance_extents')
    out['flags'] = flags
    return out


def instance_class_hist(bits, n_points, semantic, n_classes):
    """``sg_instance_class_hist`` on CUDA bit rows and a CUDA int32 / int64 label tensor [n_points], ``n_classes`` in
    1 .. 256 -> a dict of ``hist`` int32 [n, C], ``sem_label``, ``sem_count`` int32 [n] on the device.  Nothing
    synchronises.  Other inputs: numpy."""
    import torch
    if not (torch.is_tensor(bits) and bits.is_cuda):
        return instance_class_hist_numpy(bits, n_points, semantic.numpy() if torch.is_tensor(semantic) else semantic,
                                         n_classes)
    from .. import _lib as L
    n_points, n_cls = int(n_points), _n_classes(n_classes)
    bits = _bit_rows(bits, n_points, 'instance_class_hist')
    dev, n = bits.device, bits.size(0)
    if n_cls > MAX_CLASSES:
        raise L.SoftGroupHipError(f'instance_class_hist: {n_cls} classes: outside the supported range (at most '
                                  f'{MAX_CLASSES})')
    if not (torch.is_tensor(semantic) and semantic.is_cuda) or semantic.is_floating_point() \
            or semantic.numel() != n_points:
        raise ValueError(f'semantic: an integer CUDA tensor [{n_points}], one label per point of the masks')
    semantic = semantic.detach().to(dev).reshape(-1).contiguous()
    if semantic.dtype not in (torch.int32, torch.int64):
        semantic = semantic.to(torch.int64)
    with torch.cuda.device(dev):
        out = {'hist': torch.empty((n, n_cls), dtype=torch.int32, device=dev),
               'sem_label': torch.empty(n, dtype=torch.int32, device=dev),
               'sem_count': torch.empty(n, dtype=torch.int32, device=dev)}
        L.check(L.lib().sg_instance_class_hist(L.ptr(bits) if bits.numel() else None, n, n_points,
                                               L.ptr(semantic) if n_points else None,
                                               int(semantic.dtype == torch.int64), n_cls,
                                               L.ptr(out['hist']) if n else None, L.ptr(out['sem_label']),
                                               L.ptr(out['sem_count']), L.stream()), 'sg_instance_class_hist')
    return out
