"""A large cloud cut into overlapping tiles in x and y, each to be scanned at full resolution; what
``softgroup_amd.util.stitch_results`` joins again.  The reference cuts blocks offline
(dataset/stpls3d/prepare_data_inst_instance_stpls3d.py) and evaluates each as a scene of its own.

The rules (core cell ``floor((float64(x) - o) / size)``, tiles = the cells with a core point in ascending
``(cy, cx)`` order, overlap ``x < lo + margin`` / ``x >= hi - margin`` per axis, ascending point lists) are those of
``softgroup_amd.ops.stitch`` and include/softgroup_hip.h.  z is never split.
"""
import numpy as np

from ..ops import stitch as ST

__all__ = ['tile_cloud', 'TileSet']


class TileSet:
    """``point_ids``: one ascending int64 list per tile (views of one array; what ``apply_sample`` takes);
    ``core_tile`` / ``core_pos`` [n_points]: the tile that owns every point and the point's position in that
    tile's list; ``cells`` int32 [T, 2] = (cx, cy); ``tile_off`` int64 [T + 1]; ``size``, ``margin``, ``origin``.
    CUDA tensors when the cloud was one, numpy arrays otherwise."""

    def __init__(self, cells, tile_off, tile_points, core_tile, core_pos, size, margin, origin):
        import torch
        self.cells, self.core_tile, self.core_pos = cells, core_tile, core_pos
        self.tile_points = tile_points.long() if torch.is_tensor(tile_points) else tile_points.astype(np.int64)
        self.tile_off = tile_off
        self.size, self.margin, self.origin = float(size), float(margin), (float(origin[0]), float(origin[1]))
        self.n_points = int(core_tile.shape[0])
        off = tile_off.cpu().tolist() if torch.is_tensor(tile_off) else tile_off.tolist()
        self.offsets = off
        self.point_ids = [self.tile_points[off[t]:off[t + 1]] for t in range(len(off) - 1)]
        self._cells_host = None

    def __len__(self):
        return len(self.point_ids)

    @property
    def is_cuda(self):
        import torch
        return torch.is_tensor(self.core_tile) and self.core_tile.is_cuda

    def cells_host(self):
        import torch
        if self._cells_host is None:
            c = self.cells.cpu().numpy() if torch.is_tensor(self.cells) else np.asarray(self.cells)
            self._cells_host = c.astype(np.int64).reshape(-1, 2)
        return self._cells_host

    def neighbours(self):
        """the tile pairs (a < b) whose cells differ by at most 1 on both axes, ascending"""
        where = {(int(cx), int(cy)): t for t, (cx, cy) in enumerate(self.cells_host().tolist())}
        out = []
        for a, (cx, cy) in enumerate(self.cells_host().tolist()):
            for dx, dy in ((1, 0), (-1, 1), (0, 1), (1, 1)):
                b = where.get((cx + dx, cy + dy))
                if b is not None:
                    out.append((min(a, b), max(a, b)))
        return sorted(out)


def tile_cloud(xyz, size=25.0, margin=2.5, origin=None, backend='auto'):
    """-> ``TileSet`` of the cloud ``xyz`` [n, 3]: tiles of ``size`` x ``size`` in x and y that overlap their
    neighbours by ``margin`` on every side (``0 <= margin <= size / 2``); ``origin`` = (ox, oy), None = the per-axis
    minimum.  CUDA tensors in give CUDA tensors out, numpy in gives numpy out.  ``backend``: ``'device'`` (HIP
    kernels; numpy input is uploaded), ``'numpy'``, or ``'auto'`` (``ops.stitch._AUTO['tiles']``; numpy beyond the
    device's 2**29 points).  On the device: the read-backs of ``ops.stitch.tile_assign`` and one of the T + 1 tile
    offsets, which cut the views.  A coordinate that is not finite, a cell index at or beyond 2**30 and more than
    65 535 tiles raise ``ValueError``."""
    import torch

    from ..ops import resample as RS
    chosen = ST.auto_backend(backend, 'tiles')
    is_tensor = torch.is_tensor(xyz)
    is_cuda = is_tensor and xyz.is_cuda
    if chosen == 'device' and backend == 'auto' and int(xyz.shape[0]) >= ST.MAX_DEVICE_POINTS:
        chosen = 'numpy'
    if chosen == 'device':
        if not torch.cuda.is_available():
            raise RuntimeError("tile_cloud: backend='device' without a GPU")
        d_xyz = xyz if is_cuda else RS._upload(RS._xyz_numpy(xyz))
        out = ST.tile_assign(d_xyz, size, margin, origin)
        arrays, origin = out[:5], out[5]
        if not is_cuda:
            arrays = [a.cpu() for a in arrays]
            if not is_tensor:
                arrays = [a.numpy() for a in arrays]
    else:
        out = ST.tile_assign_numpy(xyz, size, margin, origin)
        arrays, origin = out[:5], out[5]
        if is_tensor:
            arrays = [torch.from_numpy(a).to(xyz.device) for a in arrays]
    return TileSet(*arrays, size, margin, origin)
