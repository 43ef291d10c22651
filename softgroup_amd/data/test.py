"""Test-time data transform: the reference's test-time ``__getitem__`` -- ``transform_test``, ``getCroppedInstLabel``
and ``getInstanceInfo`` (data/custom.py:162-194), S3DIS's ``x4_split`` (s3dis.py:46-78) and KITTI's label decode
and rank relabel (kitti.py:62-90) -- on the device, and the S3DIS test-time ``collate_fn`` (s3dis.py:80-115) over
resident items.

``TestTransform(voxel_cfg, dataset)(xyz, rgb, semantic_label, instance_label, scan_id)`` returns the item tuple of
``scan_item``, value for value and dtype for dtype, with every tensor on the device; the instance point counts
(int64) and classes (the semantic labels' dtype) are device tensors too.  Kernels of train_data.hip, all on the
current stream:

  * without the split: sg_train_augment (the fixed 0.35 pi rotation in float64, extrema keys), sg_train_compact
    (every point kept: coord = trunc(xyz_middle * scale - min)), sg_train_id_set / sg_train_remap (fill_gaps or
    rank, the map built on the host from the sorted id set), sg_train_instance_info;
  * ``x4_split``: sg_test_x4_minima (the twelve per-piece minima and a non-finite flag), sg_test_x4_split
    (piece-major rows), then the same relabel and instance statistics;
  * ``label_words=`` (KITTI): sg_kitti_decode_labels through a dense table of the learning map.

The host reads back the extrema keys (with the flags in the same copy) and the instance-id set.  A non-finite
coordinate makes the item come from ``scan_item`` on the host, an empty scan raises ``ValueError`` (the
reference's ``xyz.min(0)``), a label word whose key the learning map lacks raises the reference's ``KeyError``.
``device='cpu'`` is ``scan_item``.
"""
import math

import numpy as np
import torch

from .. import _lib as L
from ..ops import voxelization_idx
from . import scan_item
from ._train_device import _decode, _on, collate_train_device, decode_words, raise_missing_key, relabel_ids
from .train import _TYPE_TO_DATASET, PRESETS, _cfg, _KittiMap

_THETA = 0.35 * math.pi
# dataAugment(xyz, False, False, False, False): np.eye(3) @ the fixed rotation (custom.py:103-107)
_ROT = np.ascontiguousarray(np.matmul(np.eye(3), [[math.cos(_THETA), math.sin(_THETA), 0],
                                                  [-math.sin(_THETA), math.cos(_THETA), 0], [0, 0, 1]]), np.float64)
# the per-item block read back once: extrema keys, then these slots
_NONFINITE, _MISSING, _FIRST = 12, 13, 14
_EMPTY = 'zero-size array to reduction operation minimum which has no identity'


def _dtype(v):
    """torch dtype of an array or tensor"""
    if isinstance(v, torch.Tensor):
        return v.dtype
    return torch.from_numpy(np.empty(0, np.asarray(v).dtype)).dtype


def _host(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def _resident(item, dev):
    """a host item (scan_item's) with its tensors and lists on the device"""
    sid, coord, cf, feat, sem, inst, k, pointnum, cls, off = item
    cls = torch.from_numpy(np.asarray(cls, dtype=sem.numpy().dtype).reshape(-1))
    return (sid, coord.to(dev), cf.to(dev), feat.to(dev), sem.to(dev), inst.to(dev), k,
            torch.as_tensor(pointnum, dtype=torch.int64).to(dev), cls.to(dev), off.to(dev))


class TestTransform:
    """The reference's test-time ``__getitem__`` as one transform (module docstring).

    ``voxel_cfg``: ``scale`` and ``spatial_shape`` (attributes or keys).  ``dataset``: 'scannetv2' | 's3dis' |
    'stpls3d' | 'kitti' (class shift and relabel from ``train.PRESETS``).  ``x4_split``: S3DIS's four
    interleaved sub-clouds.  ``learning_map``: the ``learning_map`` table of semantic-kitti.yaml (as in the
    file, before the dataset's remap), needed for ``label_words=``.  ``device``: a GPU, or 'cpu' for
    ``scan_item``."""

    __test__ = False          # (not a pytest class)

    def __init__(self, voxel_cfg, dataset='scannetv2', x4_split=False, learning_map=None, device='cuda'):
        if dataset not in PRESETS:
            raise ValueError(f'unknown dataset {dataset!r}: one of {sorted(PRESETS)}')
        self.voxel_cfg = voxel_cfg
        self.dataset = dataset
        self.preset = dict(PRESETS[dataset])
        self.x4_split = bool(x4_split) and dataset == 's3dis'
        self.kitti = _KittiMap(learning_map)
        self.device = torch.device(device)
        self.scale = _cfg(voxel_cfg, 'scale')
        self.min_spatial = int(_cfg(voxel_cfg, 'spatial_shape')[0])

    @classmethod
    def from_config(cls, data_cfg, **kw):
        """from ``cfg.data.test`` (type, voxel_cfg, x4_split)"""
        get = (lambda k, d=None: data_cfg.get(k, d)) if isinstance(data_cfg, dict) else \
            (lambda k, d=None: getattr(data_cfg, k, d))
        kw.setdefault('x4_split', bool(get('x4_split', False)))
        return cls(get('voxel_cfg'), dataset=_TYPE_TO_DATASET[get('type')], **kw)

    def __call__(self, xyz, rgb, semantic_label=None, instance_label=None, scan_id='scan', label_words=None):
        if label_words is None and (semantic_label is None or instance_label is None):
            raise ValueError('semantic_label and instance_label, or label_words, are required')
        if self.device.type == 'cpu':
            return self._run_host(xyz, rgb, semantic_label, instance_label, scan_id, label_words)
        with torch.cuda.device(self.device):
            return self._run_device(xyz, rgb, semantic_label, instance_label, scan_id, label_words)

    def _run_host(self, xyz, rgb, sem, inst, scan_id, words):
        if words is not None:
            sem, inst = self.kitti.labels(words)
        return scan_item(_host(xyz), _host(rgb), _host(sem), _host(inst), scale=self.scale, scan_id=scan_id,
                         cls_shift=self.preset['cls_shift'], x4_split=self.x4_split, relabel=self.preset['relabel'])

    def collate(self, scans, device=None):
        """``scans``: (xyz, rgb, semantic_label, instance_label, scan_id) tuples or dicts of ``__call__``'s
        keywords -> the batch dict of the reference ``collate_fn`` (S3DIS x4: its test-time branch).  Serves as
        the ``collate=`` of ``prefetch_device``: the transform then runs on the loader thread's stream."""
        items = [self(**s) if isinstance(s, dict) else self(*s) for s in scans]
        dev = self.device if device is None else device
        if self.x4_split:
            return collate_x4_test_device(items, self.min_spatial, dev)
        return collate_train_device(items, self.min_spatial, dev)

    # ---- device --------------------------------------------------------------------------------------
    def _run_device(self, xyz, rgb, sem, inst, scan_id, words):
        dev = torch.device('cuda', torch.cuda.current_device())
        lib = L.lib()
        n = int(xyz.shape[0])
        if n == 0 or (self.x4_split and n < 4):      # (x4: a piece without points)
            raise ValueError(_EMPTY)
        xyz_d = _on(dev, xyz, torch.float32).reshape(n, 3)
        rgb_d = _on(dev, rgb, torch.float32).reshape(n, -1)
        c = rgb_d.shape[1]
        block = torch.empty(16, dtype=torch.int64, device=dev)
        if words is not None:
            sem_d, inst_d = decode_words(dev, words, self.kitti.lut(dev), block[_MISSING:_MISSING + 1])
            sem_dtype, inst_dtype = torch.int64, torch.int32          # (kitti_labels' dtypes)
        else:
            sem_d = _on(dev, sem, torch.int64).reshape(n)
            inst_d = _on(dev, inst, torch.int64).reshape(n)
            sem_dtype, inst_dtype = _dtype(sem), _dtype(inst)
        rank = self.preset['relabel'] == 'rank'
        if rank:                                   # (the first label decides the dtype of the ranked labels)
            block[_FIRST:_FIRST + 1].copy_(inst_d[:1])
        coord = torch.empty((n, 4 if self.x4_split else 3), dtype=torch.int64, device=dev)
        mid = torch.empty((n, 3), dtype=torch.float64, device=dev)
        feat = torch.empty((n, c), dtype=torch.float32, device=dev)
        sem_out = torch.empty(n, dtype=torch.int64, device=dev)
        inst_out = torch.empty(n, dtype=torch.int64, device=dev)
        if self.x4_split:
            L.check(lib.sg_test_x4_minima(L.ptr(xyz_d), n, _ROT.ctypes.data, float(self.scale), L.ptr(block),
                                          L.stream()), 'sg_test_x4_minima')
            h = block.cpu().numpy()                 # (read-back: the extrema keys and the flags)
            self._check_words(h, words)
            if h[_NONFINITE]:
                return self._fallback(xyz, rgb, sem, inst, scan_id, words, dev)
            mins = np.ascontiguousarray(_decode(h[:12]))
            L.check(lib.sg_test_x4_split(L.ptr(xyz_d), L.ptr(rgb_d), c, L.ptr(sem_d), L.ptr(inst_d), n,
                                         _ROT.ctypes.data, float(self.scale), mins.ctypes.data, L.ptr(coord),
                                         L.ptr(mid), L.ptr(feat), L.ptr(sem_out), L.ptr(inst_out), L.stream()),
                    'sg_test_x4_split')
        else:
            work = torch.empty((n, 3), dtype=torch.float64, device=dev)
            mid_in = torch.empty((n, 3), dtype=torch.float64, device=dev)
            L.check(lib.sg_train_augment(L.ptr(xyz_d), n, 0, 1.0, _ROT.ctypes.data, float(self.scale), 1.0,
                                         L.ptr(mid_in), L.ptr(work), L.ptr(block), L.stream()), 'sg_train_augment')
            h = block.cpu().numpy()                 # (read-back: the extrema keys and the flags)
            self._check_words(h, words)
            keys = _decode(h[:9])
            if not np.isfinite(keys[0:3]).all():    # (max |x| not finite: some coordinate is not)
                return self._fallback(xyz, rgb, sem, inst, scan_id, words, dev)
            mn = np.ascontiguousarray(keys[3:6])
            total = torch.empty(1, dtype=torch.int32, device=dev)
            ws = L.workspace(lib.sg_train_compact_workspace_bytes(n), dev)
            L.check(lib.sg_train_compact(L.ptr(work), L.ptr(mid_in), L.ptr(rgb_d), c, None, L.ptr(sem_d), L.ptr(inst_d),
                                         n, 1.0, mn.ctypes.data, None, n, L.ptr(coord), L.ptr(mid), L.ptr(feat),
                                         L.ptr(sem_out), L.ptr(inst_out), L.ptr(total), L.ptr(ws), ws.numel(),
                                         L.stream()), 'sg_train_compact')
        k, ids, mapped = relabel_ids(inst_out, self.preset['relabel'], dev)
        n_inst = max(int(mapped.max()) + 1, 0) if k else 0
        pointnum = torch.empty(n_inst, dtype=torch.int32, device=dev)
        cls = torch.empty(n_inst, dtype=torch.int64, device=dev)
        pt_offset = torch.empty((n, 3), dtype=torch.float64, device=dev)
        ws = L.workspace(lib.sg_train_instance_workspace_bytes(n, n_inst), dev)
        L.check(lib.sg_train_instance_info(L.ptr(mid), L.ptr(inst_out), L.ptr(sem_out), n, n_inst,
                                           int(self.preset['cls_shift']), L.ptr(pointnum), L.ptr(cls),
                                           L.ptr(pt_offset), L.ptr(ws), ws.numel(), L.stream()),
                'sg_train_instance_info')
        # dtypes as scan_item's: labels as loaded; KITTI's rank gives int64 unless the first point is unlabelled
        out_inst = inst_dtype if not rank or h[_FIRST] == -100 else torch.int64
        return (scan_id, coord, mid, feat, sem_out.to(sem_dtype), inst_out.to(out_inst), n_inst,
                pointnum.to(torch.int64), cls.to(sem_dtype), pt_offset)

    def _check_words(self, h, words):
        if words is not None and h[_MISSING] != -1:
            raise_missing_key(words, h[_MISSING])

    def _fallback(self, xyz, rgb, sem, inst, scan_id, words, dev):
        """a non-finite coordinate: the item of scan_item, moved to the device"""
        return _resident(self._run_host(xyz, rgb, sem, inst, scan_id, words), dev)


def collate_x4_test_device(items, min_spatial=128, device='cuda'):
    """The S3DIS test-time ``collate_fn`` (s3dis.py:80-115) over a device-resident x4 item (what
    ``TestTransform(..., x4_split=True)`` returns): the dict of ``collate_x4_device``, quirks included -- no
    ``coords``, ``batch_idxs`` all zero, ``batch_size`` 4, the instance lists with a leading dimension.  The
    tensors stay on the device; ``spatial_shape`` reads back the coordinate maximum (3 values)."""
    (scan_id, coord, coord_float, feat, semantic_label, instance_label, inst_num, inst_pointnum, inst_cls,
     pt_offset_label) = items[0]
    dev = torch.device(device)
    coord = coord.to(dev).long().contiguous()
    out = {
        'scan_ids': [scan_id],
        'batch_idxs': torch.zeros(coord.shape[0], dtype=torch.int32, device=dev),
        'coords_float': coord_float.to(dev).to(torch.float32),
        'feats': feat.to(dev).float(),
        'semantic_labels': semantic_label.to(dev).long(),
        'instance_labels': instance_label.to(dev).long(),
        'instance_pointnum': torch.as_tensor(inst_pointnum, dtype=torch.int32).to(dev).reshape(1, -1),
        'instance_cls': torch.as_tensor(inst_cls, dtype=torch.int64).to(dev).reshape(1, -1),
        'pt_offset_labels': pt_offset_label.to(dev).float(),
        'spatial_shape': np.clip(coord[:, 1:].max(0)[0].cpu().numpy() + 1, min_spatial, None),
        'batch_size': 4,
    }
    voxel_coords, v2p_map, p2v_map = voxelization_idx(coord, 4)
    out.update(voxel_coords=voxel_coords, v2p_map=v2p_map, p2v_map=p2v_map)
    return out
