"""Device side of ``TrainTransform`` (data/train.py) and ``collate_train_device``.

Every kernel of train_data.hip is enqueued on torch's current stream.  The host reads back, per scan:
the augmentation's extrema (bb of the first grid, or the min / room range), the extrema after each elastic
pass, the crop counts of each speculative round of candidates, and the instance-id set (plus the id set of
the S3DIS subsample).  Nothing else synchronises.
"""
import numpy as np
import torch

from .. import _lib as L
from .. import ops

_ID_PREFIX = 512                      # ids read back with the count in one copy (more: a second copy)
_ID_CAP = 8192


def _decode(keys):
    """order-preserving uint64 keys (train_data.hip dkey) -> float64"""
    k = np.ascontiguousarray(keys, np.int64).view(np.uint64)
    top = np.uint64(1) << np.uint64(63)
    bits = np.where(k & top, k ^ top, ~k)
    return bits.view(np.float64)


def _on(dev, v, dtype):
    if isinstance(v, torch.Tensor):
        v = v.to(dev)
        return v.contiguous() if v.dtype == dtype else v.to(dtype).contiguous()
    a = np.asarray(v)
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dev).to(dtype).contiguous() if t.dtype != dtype else t.to(dev).contiguous()


def relabel_ids(lab, mode, dev):
    """getCroppedInstLabel on the device (``mode`` 'fill_gaps' or 'rank'), in place on the int64 labels: id set
    (read back), map built on the host, one remap pass -> (number of ids, sorted ids, their new values)"""
    lib, n = L.lib(), lab.shape[0]
    meta = torch.empty(1 + _ID_CAP, dtype=torch.int64, device=dev)
    ws = L.workspace(lib.sg_train_id_set_workspace_bytes(), dev)
    L.check(lib.sg_train_id_set(L.ptr(lab), n, -100, L.ptr(meta), _ID_CAP, L.ptr(ws), ws.numel(), L.stream()),
            'sg_train_id_set')
    head = meta[:1 + _ID_PREFIX].cpu().numpy()       # (read-back: the instance-id set)
    k = int(head[0])
    if k > _ID_CAP:
        raise L.SoftGroupHipError(f'more than {_ID_CAP} instance ids in one scan')
    ids = head[1:1 + k] if k <= _ID_PREFIX else meta[1:1 + k].cpu().numpy()
    ids = np.sort(ids)
    from .train import fill_gaps_map, rank_map
    mapped = fill_gaps_map(ids) if mode == 'fill_gaps' else rank_map(ids)
    if k and not np.array_equal(ids, mapped):
        d = torch.from_numpy(np.concatenate([ids, mapped]).astype(np.int64)).to(dev)
        L.check(lib.sg_train_remap(L.ptr(lab), n, L.ptr(d[:k]), L.ptr(d[k:]), k, L.stream()), 'sg_train_remap')
    return k, ids, mapped


def decode_words(dev, words, lut, missing):
    """KITTI label words (int32, a ``.label`` file) -> (semantic, instance) int64 labels on the device through
    the learning map's table ``lut`` (data.kitti_lut, resident); ``missing`` (one int64 slot) receives the first
    index whose key the map lacks, -1 when none does"""
    w = _on(dev, words, torch.int32).reshape(-1)
    n = w.shape[0]
    sem = torch.empty(n, dtype=torch.int64, device=dev)
    inst = torch.empty(n, dtype=torch.int64, device=dev)
    L.check(L.lib().sg_kitti_decode_labels(L.ptr(w), n, L.ptr(lut), L.ptr(sem), L.ptr(inst), L.ptr(missing),
                                           L.stream()), 'sg_kitti_decode_labels')
    return sem, inst


def raise_missing_key(words, index):
    """dict.__getitem__'s KeyError of the reference's np.vectorize over the learning map"""
    w = words[int(index)]
    raise KeyError(int(w.item() if isinstance(w, torch.Tensor) else w) & 0xFFFF)


class _DeviceRun:
    def __init__(self, tf, rs):
        self.tf, self.rs = tf, rs
        self.words = None
        self.dev = torch.device('cuda', torch.cuda.current_device())
        self.lib = L.lib()

    def _stats(self, t):
        raw = t.cpu().numpy()                            # (read-back: the extrema; slot 9: the KITTI decode's)
        if self.words is not None and raw[9] != -1:
            raise_missing_key(self.words, raw[9])
        h = _decode(raw[:9])
        return h[0:3], h[3:6], h[6:9]

    def _ws(self, nbytes):
        return L.workspace(nbytes, self.dev)

    def relabel(self, lab, mode):
        """getCroppedInstLabel on the device: id set (read back), map built on the host, one remap pass"""
        return relabel_ids(lab, mode, self.dev)[0]

    def run(self, xyz, rgb, sem, inst, words=None):
        tf, rs, lib, dev = self.tf, self.rs, self.lib, self.dev
        xyz = _on(dev, xyz, torch.float32).reshape(-1, 3)
        n = xyz.shape[0]
        rgb = _on(dev, rgb, torch.float32).reshape(n, -1)
        stats = torch.empty(10, dtype=torch.int64, device=dev)
        self.words = words
        if words is not None:                # KITTIDataset.load's decode (kitti.py:65-72); checked at the first read-back
            sem, inst = decode_words(dev, words, tf.kitti.lut(dev), stats[9:10])
        sem = _on(dev, sem, torch.int64).reshape(n)
        inst = _on(dev, inst, torch.int64).reshape(n)
        c = rgb.shape[1]
        if tf.x4_split:                    # S3DISDataset.load (s3dis.py:31-41)
            m = int(n * 0.25)
            if tf.rng == 'numpy':
                idx = torch.from_numpy(rs.choice_host(n, m).astype(np.int64)).to(dev)
            else:
                idx = rs.choice_device(n, m).contiguous()
            outs = (torch.empty((m, 3), dtype=torch.float32, device=dev), torch.empty((m, c), dtype=torch.float32, device=dev),
                    torch.empty(m, dtype=torch.int64, device=dev), torch.empty(m, dtype=torch.int64, device=dev))
            L.check(lib.sg_train_gather(L.ptr(idx), m, L.ptr(xyz), L.ptr(rgb), c, L.ptr(sem), L.ptr(inst),
                                        *[L.ptr(o) for o in outs], L.stream()), 'sg_train_gather')
            xyz, rgb, sem, inst = outs
            n = m
            self.relabel(inst, 'fill_gaps')
        down = float(tf.preset['down'])
        mat, sf = tf._augment_draws(rs)
        elastic = rs.rand() < tf.aug_prob
        mat = np.ascontiguousarray(mat, np.float64)
        xyz_middle = torch.empty((n, 3), dtype=torch.float64, device=dev)
        work = torch.empty((n, 3), dtype=torch.float64, device=dev)
        L.check(lib.sg_train_augment(L.ptr(xyz), n, int(sf is not None), float(sf or 1.0), mat.ctypes.data,
                                     float(tf.scale), down, L.ptr(xyz_middle), L.ptr(work), L.ptr(stats),
                                     L.stream()), 'sg_train_augment')
        amax, mn, mx = self._stats(stats)
        if elastic:
            for gran, mag in ((6, 40.), (20, 160.)):
                bb = amax.astype(np.int32) // gran + 3
                if tf.rng == 'numpy':
                    grids = torch.from_numpy(np.stack([rs.grid_host(bb) for _ in range(3)])).to(dev)
                else:
                    grids = rs.grid_device(bb)
                tmp = torch.empty_like(grids)
                b0, b1, b2 = (int(b) for b in bb)
                L.check(lib.sg_train_blur(L.ptr(grids), L.ptr(tmp), b0, b1, b2, 3, L.stream()), 'sg_train_blur')
                L.check(lib.sg_train_elastic(L.ptr(work), n, L.ptr(grids), b0, b1, b2, float(gran), mag / down,
                                             L.ptr(stats), L.stream()), 'sg_train_elastic')
                amax, mn, mx = self._stats(stats)
        if down != 1:
            mn, mx = mn * down, mx * down             # (x * down is monotonic: its extrema are these)
        room = (mx - mn) - (mn - mn)
        mn = np.ascontiguousarray(mn, np.float64)
        counts = torch.empty(16, dtype=torch.int64, device=dev)

        def count(cands):
            cand = np.ascontiguousarray([np.concatenate([o, s.astype(np.float64)]) for o, s in cands], np.float64)
            L.check(lib.sg_train_crop_count(L.ptr(work), n, down, mn.ctypes.data, cand.ctypes.data, len(cands),
                                            L.ptr(counts), L.stream()), 'sg_train_crop_count')
            return counts[:len(cands)].cpu().numpy().tolist()       # (read-back: the crop counts)

        got = tf._crop(rs, n, room, count)
        if got is None:
            return None
        off, shape, kept = got
        crop = None if off is None else np.ascontiguousarray(np.concatenate([off, shape.astype(np.float64)]))
        noise = torch.from_numpy(np.ascontiguousarray(rs.feat_noise(c), np.float32)).to(dev)
        coord = torch.empty((kept, 3), dtype=torch.int64, device=dev)
        mid_out = torch.empty((kept, 3), dtype=torch.float64, device=dev)
        feat = torch.empty((kept, c), dtype=torch.float32, device=dev)
        sem_out = torch.empty(kept, dtype=torch.int64, device=dev)
        inst_out = torch.empty(kept, dtype=torch.int64, device=dev)
        total = torch.empty(1, dtype=torch.int32, device=dev)
        ws = self._ws(lib.sg_train_compact_workspace_bytes(n))
        L.check(lib.sg_train_compact(L.ptr(work), L.ptr(xyz_middle), L.ptr(rgb), c, L.ptr(noise), L.ptr(sem),
                                     L.ptr(inst), n, down, mn.ctypes.data, None if crop is None else crop.ctypes.data, kept,
                                     L.ptr(coord), L.ptr(mid_out), L.ptr(feat), L.ptr(sem_out), L.ptr(inst_out),
                                     L.ptr(total), L.ptr(ws), ws.numel(), L.stream()), 'sg_train_compact')
        k = self.relabel(inst_out, tf.preset['relabel'])
        pointnum = torch.empty(k, dtype=torch.int32, device=dev)
        cls = torch.empty(k, dtype=torch.int64, device=dev)
        pt_offset = torch.empty((kept, 3), dtype=torch.float64, device=dev)
        ws = self._ws(lib.sg_train_instance_workspace_bytes(kept, k))
        L.check(lib.sg_train_instance_info(L.ptr(mid_out), L.ptr(inst_out), L.ptr(sem_out), kept, k,
                                           int(tf.preset['cls_shift']), L.ptr(pointnum), L.ptr(cls), L.ptr(pt_offset),
                                           L.ptr(ws), ws.numel(), L.stream()), 'sg_train_instance_info')
        return coord, mid_out, feat, sem_out, inst_out, k, pointnum, cls, pt_offset


def collate_train_device(items, min_spatial=128, device='cuda'):
    """The reference ``collate_fn`` (custom.py:196-256) over device-resident training items (what
    ``TrainTransform`` returns): same keys, dtypes and values; ``None`` items skipped; instance ids shifted by
    the running instance total.  The tensors stay on the device; ``spatial_shape`` reads back the coordinate
    maximum (3 values).  Items are expected on the current stream (made there, or waited for)."""
    dev = torch.device(device)
    scan_ids, coords, cf, feats, sem, ins, pointnum, cls, offs = [], [], [], [], [], [], [], [], []
    total, b = 0, 0
    for it in items:
        if it is None:
            continue
        (scan_id, coord, coord_float, feat, semantic_label, instance_label, inst_num, inst_pointnum,
         inst_cls, pt_offset_label) = it
        coord = coord.to(dev)
        instance_label = instance_label.to(dev).long()
        if total:
            instance_label = torch.where(instance_label != -100, instance_label + total, instance_label)
        total += int(inst_num)
        scan_ids.append(scan_id)
        coords.append(torch.cat([torch.full((coord.shape[0], 1), b, dtype=torch.int64, device=dev), coord.long()], 1))
        cf.append(coord_float.to(dev))
        feats.append(feat.to(dev))
        sem.append(semantic_label.to(dev))
        ins.append(instance_label)
        pointnum.append(torch.as_tensor(inst_pointnum, dtype=torch.int32).to(dev))
        cls.append(torch.as_tensor(inst_cls, dtype=torch.int64).to(dev))
        offs.append(pt_offset_label.to(dev))
        b += 1
    assert b > 0, 'empty batch'
    d_coords = torch.cat(coords, 0)
    out = {
        'scan_ids': scan_ids,
        'coords': d_coords,
        'batch_idxs': d_coords[:, 0].int(),
        'coords_float': torch.cat(cf, 0).to(torch.float32),
        'feats': torch.cat(feats, 0).float(),
        'semantic_labels': torch.cat(sem, 0).long(),
        'instance_labels': torch.cat(ins, 0).long(),
        'instance_pointnum': torch.cat(pointnum).int(),
        'instance_cls': torch.cat(cls).long(),
        'pt_offset_labels': torch.cat(offs).float(),
        'spatial_shape': np.clip(d_coords[:, 1:].max(0)[0].cpu().numpy() + 1, min_spatial, None),
        'batch_size': b,
    }
    voxel_coords, v2p_map, p2v_map = ops.voxelization_idx(d_coords, b)
    out.update(voxel_coords=voxel_coords, v2p_map=v2p_map, p2v_map=p2v_map)
    return out
