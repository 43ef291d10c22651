"""Superpoints where a dataset ships none: ``make_superpoints`` composes ``ops.geometry.knn``, ``point_normals`` and
``grow_segments`` into the id array that ``superpoint_index`` / ``refine_result`` / ``snap_instances`` accept as it is.

The method is region growing over kNN links by normal angle (and, if asked, curvature and distance) -- the idea of
PCL's region growing without its seed order, which is what makes it order-free and parallel: a segment is a connected
component of the links, whatever the order the points come in.  It is NOT the Felzenszwalb mesh segmentation that
produced ScanNet's ``*.segs.json``; links are transitive, so a gently curved surface can chain into one segment.
"""
from ..ops import geometry as G

__all__ = ['make_superpoints']


def make_superpoints(xyz, k=16, angle=10.0, max_curvature=None, max_dist=None, min_size=20, small='absorb', cell=None,
                     backend='auto', return_geometry=False):
    """-> sp int32 [n]: a superpoint id per point (-1 = in none), numbered in ascending order of each segment's
    smallest point.  ``xyz`` [n, 3]: a CUDA tensor stays on the device from start to end (CUDA tensor out); numpy
    arrays and CPU tensors give numpy out, through the device or the numpy twins as ``backend`` says per operation.

    k, cell, max_dist: of the neighbour search (``max_dist`` also bounds a link's length);
    angle (degrees), max_curvature, min_size, small: of ``grow_segments``.
    With ``return_geometry`` -> (sp, normals float32 [n, 3], curvature float32 [n], nbr_idx int32 [n, k])."""
    if not G._is_cuda(xyz) and all(G.auto_backend(backend, op) == 'device' for op in ('knn', 'normals', 'grow')):
        # one upload, the three steps on the device, one download
        out = make_superpoints(G._upload(G._xyz_numpy(xyz)), k, angle, max_curvature, max_dist, min_size, small, cell,
                               'device', return_geometry)
        return tuple(o.cpu().numpy() for o in out) if return_geometry else out.cpu().numpy()
    nbr_idx, nbr_d2 = G.knn(xyz, k, cell=cell, max_dist=max_dist, backend=backend)
    normals, curvature = G.point_normals(xyz, nbr_idx, backend=backend)
    sp, _ = G.grow_segments(nbr_idx, normals, curvature if max_curvature is not None else None,
                            nbr_d2 if max_dist is not None else None, angle=angle, max_curvature=max_curvature,
                            max_dist=max_dist, min_size=min_size, small=small, backend=backend)
    return (sp, normals, curvature, nbr_idx) if return_geometry else sp
