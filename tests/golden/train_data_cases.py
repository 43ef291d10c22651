"""The cases of tests/golden/ref_train_data.npz (make_ref_train_data.py): the synthetic raw scans, in each
dataset's file format and as its ``load`` yields them, and the configuration of each case."""
import numpy as np

from softgroup_amd import data, synthetic

NAMES = ('scan_id', 'coord', 'coord_float', 'feat', 'semantic_label', 'instance_label', 'inst_num',
         'inst_pointnum', 'inst_cls', 'pt_offset_label')
# (a subset of the SemanticKITTI table: raw label -> learning id; 1..8 things, 9..19 stuff)
KITTI_MAP = ((0, 0), (1, 0), (10, 1), (11, 2), (15, 3), (18, 4), (30, 6), (40, 9), (48, 11), (50, 13), (70, 15),
             (71, 16), (80, 18))


def _vc(scale=50, spatial=(128, 512), max_npoint=250000, min_npoint=1000):
    return dict(scale=scale, spatial_shape=list(spatial), max_npoint=max_npoint, min_npoint=min_npoint)


CASES = [
    dict(name='scannet_nocrop', dataset='scannetv2', aug_prob=1.0, voxel_cfg=_vc(), seeds=[1],
         scene=dict(n=2500, room_scale=0.14)),
    dict(name='scannet_crop', dataset='scannetv2', aug_prob=1.0, voxel_cfg=_vc(spatial=(128, 160), max_npoint=2500),
         seeds=[2], scene=dict(n=5000, room_scale=0.5)),
    dict(name='scannet_none', dataset='scannetv2', aug_prob=1.0,
         voxel_cfg=_vc(spatial=(128, 160), max_npoint=1000, min_npoint=950), seeds=[3], scene=dict(n=5000, room_scale=0.5)),
    dict(name='scannet_aug_half', dataset='scannetv2', aug_prob=0.5, voxel_cfg=_vc(), seeds=[4, 5],
         scene=dict(n=2000, room_scale=0.14)),
    dict(name='stpls3d', dataset='stpls3d', aug_prob=1.0, voxel_cfg=_vc(scale=3), seeds=[7],
         scene=dict(n=2500, room_scale=0.12)),
    dict(name='s3dis_x4', dataset='s3dis', aug_prob=1.0, x4_split=True,
         voxel_cfg=_vc(spatial=(128, 192), max_npoint=1200, min_npoint=500), seeds=[8], scene=dict(n=8000, room_scale=0.5)),
    dict(name='kitti', dataset='kitti', aug_prob=1.0, voxel_cfg=_vc(scale=20, spatial=(128, 160), max_npoint=2500),
         seeds=[9], scene=dict(n=5000, room_scale=0.12)),
    dict(name='batch', dataset='scannetv2', aug_prob=1.0, voxel_cfg=_vc(), seeds=[11, 12], batch=True,
         scene=dict(n=2000, room_scale=0.14)),
]


def raw_digest(load):
    """sha256 over the raw arrays of a scan (the golden file stores this instead of the arrays: they are
    regenerated from the synthetic scene, and the digest proves they are the inputs the reference saw)"""
    import hashlib
    h = hashlib.sha256()
    for k in ('xyz', 'rgb', 'sem', 'inst'):
        a = np.ascontiguousarray(load[k])
        h.update(f'{k}:{a.dtype.str}:{a.shape}'.encode())
        h.update(a.tobytes())
    return h.hexdigest()


def raw_case(case, j):
    """-> dict(file=<what the dataset's file holds>, load=dict(xyz, rgb, sem, inst) as its load yields them)"""
    seed = 100 + 10 * CASES.index(case) + j
    xyz, rgb, inst = synthetic.scene_s2(seed=seed, **case['scene'])
    kind = case['dataset']
    if kind == 'kitti':
        things, stuff = [10, 11, 15, 18, 30], [40, 48, 50, 70, 71, 80, 0, 1]
        cls = np.where(inst >= 0, np.array(things)[np.clip(inst, 0, None) % 5],
                       np.array(stuff)[np.arange(len(inst)) % 8])
        word = (np.where(inst >= 0, (inst * 7 + 3), 0).astype(np.int64) << 16 | cls).astype(np.int32)
        raw = np.concatenate([xyz * 8, rgb[:, :1]], 1).astype(np.float32)
        sem, lab = data.kitti_labels(word, dict(KITTI_MAP))
        return dict(file=(raw, word), load=dict(xyz=raw[:, :3].copy(), rgb=raw[:, 3:].copy(), sem=sem, inst=lab))
    inst = inst.astype(np.float64)
    if j == 1:
        inst[inst == 3] = -100                  # a gap in the ids
    if kind == 'stpls3d':
        xyz = (xyz * 20).astype(np.float32)
        sem = np.where(inst >= 0, 1 + inst % 14, 0).astype(np.float64)
    elif kind == 's3dis':
        sem = np.where(inst >= 0, inst % 13, 1).astype(np.float64)
    else:
        sem = np.where(inst >= 0, 2 + inst % 18, 0).astype(np.float64)
        sem[::97] = -100
    load = dict(xyz=xyz, rgb=rgb, sem=sem, inst=inst)
    f = (xyz, rgb, sem, inst, None, None) if kind == 's3dis' else (xyz, rgb, sem, inst)
    return dict(file=f, load=load)
