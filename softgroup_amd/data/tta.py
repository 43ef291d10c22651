"""Test-time augmentation around a scan function (host only): the transforms, their application to a cloud and the
loop that scans every transformed cloud and hands the results to ``softgroup_amd.util.ensemble_results``.  Nothing
in ``forward_test`` or ``ScanForward`` calls this; the reference has no counterpart.

A transform is a 3 x 3 matrix m applied to row vectors: ``xyz_t[:, i] = sum_j m[i, j] * xyz[:, j]``.  The transforms
of ``tta_transforms`` are SIGNED PERMUTATIONS (quarter turns about z, a mirror of x): applying one is a column swap
and a sign change, exact in any float format.  The points keep their order, which is what ``ensemble_results`` needs.
"""
import numpy as np

__all__ = ['tta_transforms', 'apply_tta', 'tta_scan']


def tta_transforms(rot90=(0, 1, 2, 3), flip_x=(False, )):
    """-> list of float64 [3, 3] signed permutation matrices: for every ``flip`` of ``flip_x`` (outer) and every
    ``r`` of ``rot90`` (inner) the mirror ``x -> -x`` (when ``flip``) followed by r quarter turns about z
    (``(x, y) -> (-y, x)`` per turn).  The identity always comes FIRST (pass 0 is the untransformed pass) and every
    matrix appears once."""
    turn = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], dtype=np.int64)
    out = [np.eye(3, dtype=np.int64)]
    for flip in flip_x:
        if flip not in (False, True, 0, 1):
            raise ValueError(f'flip_x entry {flip!r}: True or False')
        mirror = np.diag([-1 if flip else 1, 1, 1]).astype(np.int64)
        for r in rot90:
            if int(r) != r:
                raise ValueError(f'rot90 entry {r!r}: an integer number of quarter turns')
            m = np.linalg.matrix_power(turn, int(r) % 4) @ mirror
            if not any(np.array_equal(m, seen) for seen in out):
                out.append(m)
    return [m.astype(np.float64) for m in out]


def _signed_permutation(m):
    """(source column, sign) per output column, or None"""
    if not (np.isin(m, (-1.0, 0.0, 1.0)).all() and (np.abs(m).sum(0) == 1).all() and (np.abs(m).sum(1) == 1).all()):
        return None
    cols = np.abs(m).argmax(1)
    return cols, m[np.arange(3), cols]


def apply_tta(xyz, m):
    """``xyz`` [n, 3] (numpy array or torch tensor) under the 3 x 3 matrix ``m`` -> a new array of the same kind and
    dtype.  A signed permutation is applied as a column swap and a sign change: exact.  Any other matrix goes through
    float64 and is cast once."""
    m = np.asarray(m, dtype=np.float64)
    if m.shape != (3, 3) or not np.isfinite(m).all():
        raise ValueError('transform: a finite 3 x 3 matrix')
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError('xyz: an array [n, 3]')
    sp = _signed_permutation(m)
    if isinstance(xyz, np.ndarray):
        if sp is not None:
            out = np.empty_like(xyz)
            for i in range(3):
                out[:, i] = xyz[:, sp[0][i]] if sp[1][i] > 0 else -xyz[:, sp[0][i]]
            return out
        return (xyz.astype(np.float64) @ m.T).astype(xyz.dtype)
    import torch
    if sp is not None:
        return torch.stack([xyz[:, int(sp[0][i])] if sp[1][i] > 0 else -xyz[:, int(sp[0][i])] for i in range(3)], 1)
    return (xyz.double() @ torch.from_numpy(m.T.copy()).to(xyz.device)).to(xyz.dtype)


def tta_scan(run, xyz, *arrays, transforms=None, **ensemble_kw):
    """``run(xyz_t, *arrays) -> result dict`` once per transform (default ``tta_transforms()``), in order, and the
    results combined by ``ensemble_results(results, **ensemble_kw)``.  Pass 0 is the untransformed cloud: its offsets
    and coordinates are the ones the combined result keeps."""
    from ..util.ensemble import ensemble_results
    transforms = tta_transforms() if transforms is None else list(transforms)
    if not transforms:
        raise ValueError('transforms: at least one')
    return ensemble_results([run(apply_tta(xyz, m), *arrays) for m in transforms], **ensemble_kw)
