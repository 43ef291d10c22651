"""Training-time data transform: ``CustomDataset.transform_train`` + ``getInstanceInfo``
+ the training branch of ``__getitem__`` (data/custom.py:52-194, data/kitti.py:78-118, data/s3dis.py:31-44)
on the device, and the reference ``collate_fn`` (custom.py:196-256) over device-resident items.

``TrainTransform(voxel_cfg, dataset)(xyz, rgb, semantic_label, instance_label, scan_id, index)`` returns
the reference's 10-field training item (or ``None`` where it returns ``None``):

  * ``dataAugment`` (custom.py:92-111) with each dataset's argument quirk: the custom datasets pass
    ``aug_prob`` into the ``scale`` slot (custom.py:139), KITTI passes ``True, True, True, True, aug_prob``;
  * two ``elastic`` passes (custom.py:52-74): Gaussian noise grids blurred by the 3-tap box x, y, z, x, y, z
    (scipy.ndimage's arithmetic: each pass summed in float64, rounded to float32) and sampled trilinearly
    (scipy's RegularGridInterpolator: corners in ``itertools.product`` order, weights multiplied in axis
    order, 0 outside the grid); KITTI works at scale / 5 (kitti.py:92-99);
  * the random ``crop`` loop (custom.py:113-127, S3DIS step 64) and up to 5 tries (custom.py:144-154);
  * instance relabelling: ``fill_gaps`` (custom.py:129-136) or the KITTI ``rank`` (kitti.py:78-90);
  * ``getInstanceInfo`` (custom.py:76-90) with the dataset's class shift, and the feature noise (:184);
  * S3DIS ``x4_split`` training first keeps a random 25 % of the points (s3dis.py:31-41).

Two random streams:

  * ``rng='numpy'`` consumes the global ``np.random`` stream -- and ``torch``'s CPU generator for the feature
    noise -- exactly as the reference does, draw for draw: same seeds, same item.  The noise grids are drawn
    on the host (``np.random.randn``), which dominates the time of this mode.
  * ``rng='device'`` draws the scalars from a ``numpy.random.Generator`` seeded by ``(seed, index)`` and the
    noise grids and the S3DIS subsample on the device from a ``torch.Generator`` seeded the same way: an
    item depends on ``(seed, index)`` only, not on the thread or the order it was made in.

``device='cpu'`` is a numpy restatement of the same transform (no scipy) for CPU-only tooling.  On the device
everything runs in the kernels of train_data.hip on the current stream; the host reads back a few scalars
where the reference's control flow needs them ("Training data").
"""
import itertools
import math

import numpy as np
import torch

# dataset -> (class shift of getInstanceInfo, crop step, relabel, elastic down-scale)
PRESETS = {
    'scannetv2': dict(cls_shift=2, step=32, relabel='fill_gaps', down=1),
    's3dis': dict(cls_shift=0, step=64, relabel='fill_gaps', down=1),
    'stpls3d': dict(cls_shift=1, step=32, relabel='fill_gaps', down=1),
    'kitti': dict(cls_shift=11, step=32, relabel='rank', down=5),
}
_TYPE_TO_DATASET = {'scannetv2': 'scannetv2', 's3dis': 's3dis', 'stpls3d': 'stpls3d', 'kitti': 'kitti'}
_BLUR_W = float(np.float32(1) / 3)          # np.ones(..).astype('float32') / 3, read as double by scipy
_SPEC = 16                                  # crop candidates evaluated per speculative round


def _cfg(voxel_cfg, key):
    return voxel_cfg[key] if isinstance(voxel_cfg, dict) else getattr(voxel_cfg, key)


# ---------------------------------------------------------------------------------------------------------
# random streams
# ---------------------------------------------------------------------------------------------------------
class _NumpyStream:
    """the global np.random stream (and torch's CPU generator for the feature noise), as the reference"""
    def rand(self, size=None):
        return np.random.rand() if size is None else np.random.rand(size)

    def randn33(self):
        return np.random.randn(3, 3)

    def randint(self, lo, hi):
        return np.random.randint(lo, hi)

    def uniform(self, lo, hi):
        return np.random.uniform(lo, hi)

    def state(self):
        return np.random.get_state()

    def restore(self, st):
        np.random.set_state(st)

    def choice_host(self, n, m):
        return np.random.choice(n, m, replace=False)

    def grid_host(self, shape):
        return np.random.randn(*[int(b) for b in shape]).astype('float32')

    def feat_noise(self, c):
        return (torch.randn(c) * 0.1).numpy()


class _GeneratorStream:
    """rng='device': scalars from a numpy Generator, bulk draws from a torch Generator, both seeded by
    (seed, index) alone"""
    def __init__(self, seed, index, device):
        ss = np.random.SeedSequence([int(seed) & 0xFFFFFFFF, int(index) & 0xFFFFFFFF])
        s_host, s_dev = ss.spawn(2)
        self.g = np.random.Generator(np.random.PCG64(s_host))
        self.dev = device
        self.tg = None
        self.tseed = int(s_dev.generate_state(1, np.uint64)[0] & 0x7FFFFFFFFFFFFFFF)

    def rand(self, size=None):
        return self.g.random() if size is None else self.g.random(size)

    def randn33(self):
        return self.g.standard_normal((3, 3))

    def randint(self, lo, hi):
        return int(self.g.integers(lo, hi))

    def uniform(self, lo, hi):
        return self.g.uniform(lo, hi)

    def state(self):
        return self.g.bit_generator.state

    def restore(self, st):
        self.g.bit_generator.state = st

    def _torch_gen(self):
        if self.tg is None:
            self.tg = torch.Generator(device=self.dev)
            self.tg.manual_seed(self.tseed)
        return self.tg

    def choice_host(self, n, m):
        return self.g.permutation(n)[:m]

    def grid_host(self, shape):
        return self.g.standard_normal(tuple(int(b) for b in shape), dtype=np.float32)

    def choice_device(self, n, m):
        return torch.randperm(n, generator=self._torch_gen(), device=self.dev)[:m]

    def grid_device(self, shape):
        return torch.randn(3, *[int(b) for b in shape], generator=self._torch_gen(), device=self.dev)

    def feat_noise(self, c):
        return self.g.standard_normal(c, dtype=np.float32) * np.float32(0.1)


# ---------------------------------------------------------------------------------------------------------
# numpy restatements (device='cpu', and the reference for the per-stage tests)
# ---------------------------------------------------------------------------------------------------------
def blur_numpy(grid):
    """scipy.ndimage.convolve with the [1,1,1]/3 box along x, y, z, x, y, z, mode='constant', cval=0 on a
    float32 grid: each output = float32(((0 + a[i-1] w) + a[i] w) + a[i+1] w) in float64"""
    g = np.asarray(grid, np.float32)
    for axis in (0, 1, 2, 0, 1, 2):
        a = np.moveaxis(g, axis, 0).astype(np.float64)
        p = np.zeros((a.shape[0] + 2, ) + a.shape[1:])
        p[1:-1] = a
        s = ((p[:-2] * _BLUR_W + p[1:-1] * _BLUR_W) + p[2:] * _BLUR_W).astype(np.float32)
        g = np.ascontiguousarray(np.moveaxis(s, 0, axis))
    return g


def interp_numpy(grid, gran, x):
    """RegularGridInterpolator(linspace(-(b-1) gran, (b-1) gran, b) per axis, grid, bounds_error=0,
    fill_value=0)(x) for a float32 grid, in scipy 1.15's order (_rgi.py: _evaluate_linear)"""
    bb = grid.shape
    idx, nd, oob = [], [], np.zeros(x.shape[0], bool)
    for a in range(3):
        ax = np.linspace(-(bb[a] - 1) * gran, (bb[a] - 1) * gran, bb[a])
        xa = x[:, a]
        i = np.clip(np.searchsorted(ax, xa, side='right') - 1, 0, bb[a] - 2)
        idx.append(i)
        nd.append((xa - ax[i]) / (ax[i + 1] - ax[i]))
        oob |= (xa < ax[0]) | (xa > ax[-1])
    value = np.zeros(x.shape[0])
    for c in itertools.product((0, 1), repeat=3):
        w = np.ones(x.shape[0])
        for a in range(3):
            w = w * (nd[a] if c[a] else 1 - nd[a])
        value = value + grid[idx[0] + c[0], idx[1] + c[1], idx[2] + c[2]].astype(np.float64) * w
    value[oob] = 0
    return value


def fill_gaps_map(ids):
    """``getCroppedInstLabel``'s loop (custom.py:129-136) as a map over the sorted non-negative ids present:
    while an id below the current maximum is missing, the maximum moves into it"""
    ids = np.asarray(ids, np.int64)
    k = ids.size
    present = set(ids.tolist())
    holes = [j for j in range(k) if j not in present]
    big = ids[ids >= k][::-1]                  # largest first
    out = ids.copy()
    pos = {v: i for i, v in enumerate(ids.tolist())}
    for h, v in zip(holes, big.tolist()):
        out[pos[v]] = h
    return out


def rank_map(ids):
    """KITTI's getCroppedInstLabel (kitti.py:78-90): ids -> rank among the ids present"""
    return np.arange(len(ids), dtype=np.int64)


class _KittiMap:
    """the ``learning_map`` of semantic-kitti.yaml (as in the file) for ``label_words=``: decoded on the host by
    ``kitti_labels``, on the device through its dense table (``kitti_lut``, one copy per device)"""
    def __init__(self, learning_map):
        self.map = None if learning_map is None else {int(k): int(v) for k, v in dict(learning_map).items()}
        self._table, self._dev = None, {}

    def _need(self):
        if self.map is None:
            raise ValueError('label_words= needs the learning_map of semantic-kitti.yaml')

    def labels(self, words):
        from . import kitti_labels
        self._need()
        return kitti_labels(words.cpu().numpy() if isinstance(words, torch.Tensor) else np.asarray(words), self.map)

    def lut(self, dev):
        from . import kitti_lut
        self._need()
        if self._table is None:
            self._table = kitti_lut(self.map)
        t = self._dev.get(dev)
        if t is None:
            t = self._dev[dev] = torch.from_numpy(self._table).to(dev)
        return t


def _relabel_numpy(lab, mode):
    """the relabel of the reference, dtype quirks included"""
    from . import _fill_gaps, _rank_ids
    return _fill_gaps(lab) if mode == 'fill_gaps' else _rank_ids(lab)


# ---------------------------------------------------------------------------------------------------------
class TrainTransform:
    """The reference's training ``__getitem__`` as one transform (module docstring).

    ``voxel_cfg``: ``scale``, ``spatial_shape``, ``max_npoint``, ``min_npoint`` (attributes or keys).
    ``dataset``: 'scannetv2' | 's3dis' | 'stpls3d' | 'kitti'.  ``x4_split``: S3DIS training subsample.
    ``rng``: 'device' (fast, seeded by ``(seed, index)``) or 'numpy' (the reference's stream).
    ``device``: a GPU device, or 'cpu' for the numpy restatement.  ``learning_map``: the table of
    semantic-kitti.yaml, for raw KITTI ``label_words=`` (decoded by sg_kitti_decode_labels on the device)."""

    def __init__(self, voxel_cfg, dataset='scannetv2', aug_prob=1.0, x4_split=False, rng='device', seed=None,
                 device='cuda', learning_map=None):
        if dataset not in PRESETS:
            raise ValueError(f'unknown dataset {dataset!r}: one of {sorted(PRESETS)}')
        if rng not in ('device', 'numpy'):
            raise ValueError("rng must be 'device' or 'numpy'")
        self.voxel_cfg = voxel_cfg
        self.dataset = dataset
        self.preset = dict(PRESETS[dataset])
        self.aug_prob = aug_prob
        self.x4_split = bool(x4_split) and dataset == 's3dis'
        self.rng = rng
        self.seed = 0 if seed is None else int(seed)
        self.device = torch.device(device)
        self.scale = _cfg(voxel_cfg, 'scale')
        self.spatial = int(_cfg(voxel_cfg, 'spatial_shape')[1])
        self.max_npoint = _cfg(voxel_cfg, 'max_npoint')
        self.min_npoint = _cfg(voxel_cfg, 'min_npoint')
        self.trace = None          # (device='cpu': a list collects the values tested against thresholds)
        self.kitti = _KittiMap(learning_map)

    @classmethod
    def from_config(cls, data_cfg, **kw):
        """from ``cfg.data.train`` (type, voxel_cfg, x4_split, ...)"""
        get = (lambda k, d=None: data_cfg.get(k, d)) if isinstance(data_cfg, dict) else \
            (lambda k, d=None: getattr(data_cfg, k, d))
        kw.setdefault('x4_split', bool(get('x4_split', False)))
        return cls(get('voxel_cfg'), dataset=_TYPE_TO_DATASET[get('type')], **kw)

    # ---- shared control flow --------------------------------------------------------------------------
    def _stream(self, index):
        return _NumpyStream() if self.rng == 'numpy' else _GeneratorStream(self.seed, index, self.device)

    def _augment_draws(self, rs):
        """dataAugment's draws (custom.py:92-111) with the dataset's arguments -> (matrix, scale factor)"""
        p = self.aug_prob
        if self.dataset == 'kitti':      # dataAugment(xyz, True, True, True, True, aug_prob)
            jitter, flip, rot, scale, prob = True, True, True, True, p
        else:                            # dataAugment(xyz, True, True, True, aug_prob): aug_prob is `scale`
            jitter, flip, rot, scale, prob = True, True, True, p, 1.0
        m = np.eye(3)
        if jitter and rs.rand() < prob:
            m += rs.randn33() * 0.1
        if flip and rs.rand() < prob:
            m[0][0] *= rs.randint(0, 2) * 2 - 1
        if rot and rs.rand() < prob:
            theta = rs.rand() * 2 * math.pi
        else:
            theta = 0.35 * math.pi
        m = np.matmul(m, [[math.cos(theta), math.sin(theta), 0], [-math.sin(theta), math.cos(theta), 0], [0, 0, 1]])
        sf = None
        if scale and rs.rand() < prob:
            sf = rs.uniform(0.95, 1.05)
        return m, sf

    def _crop(self, rs, n, room, count, spec=_SPEC):
        """the crop tries (custom.py:113-127, 144-154): -> (offset or None, spatial shape, kept count) of the
        accepted crop, or None.  ``count(cands)`` counts the kept points of each (offset, shape) candidate.
        Candidates are drawn ahead, evaluated in one call, and the stream is then rewound and advanced by
        exactly the draws the reference makes."""
        step = self.preset['step']
        valid = n
        for _ in range(5):
            ss = np.array([self.spatial] * 3)
            valid, off, shape = n, None, None
            prev = n                       # count deciding the step of the NEXT decrement
            while valid > self.max_npoint:
                st = rs.state()
                cands, ss_k, prev_k = [], ss.copy(), prev
                for _k in range(spec):
                    o = np.clip(ss_k - room + 0.001, None, 0) * rs.rand(3)
                    cands.append((o, ss_k.copy()))
                    ss_k[:2] -= step * 2 if prev_k > 1e6 else step
                    prev_k = 0             # (speculation: later counts are not above 1e6)
                counts = count(cands)
                rs.restore(st)
                for k, c in enumerate(counts):
                    o = np.clip(ss - room + 0.001, None, 0) * rs.rand(3)
                    assert np.array_equal(o, cands[k][0]) and np.array_equal(ss, cands[k][1])
                    valid, off, shape = int(c), o, ss.copy()
                    ss[:2] -= step * 2 if prev > 1e6 else step
                    prev = valid
                    if valid <= self.max_npoint or (valid > 1e6 and k + 1 < len(counts)):
                        break       # done, or the next candidate's successor was speculated with the wrong step
            if valid >= self.min_npoint:
                return off, shape, valid
        return None

    def __call__(self, xyz, rgb, semantic_label=None, instance_label=None, scan_id='scan', index=0, label_words=None):
        """``label_words``: the int32 words of a KITTI ``.label`` file instead of the two label arrays"""
        rs = self._stream(index)
        if self.device.type == 'cpu':
            if label_words is not None:
                semantic_label, instance_label = self.kitti.labels(label_words)
            out = self._run_cpu(rs, xyz, rgb, semantic_label, instance_label)
        else:
            with torch.cuda.device(self.device):
                out = self._run_device(rs, xyz, rgb, semantic_label, instance_label, label_words)
        if out is None:
            return None
        return (scan_id, ) + out

    # ---- numpy ---------------------------------------------------------------------------------------
    def _run_cpu(self, rs, xyz, rgb, sem, inst):
        xyz, rgb, sem, inst = (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
                               for v in (xyz, rgb, sem, inst))
        if self.x4_split:                  # S3DISDataset.load (s3dis.py:31-41)
            n0 = xyz.shape[0]
            inds = rs.choice_host(n0, int(n0 * 0.25))
            xyz, rgb, sem = xyz[inds], rgb[inds], sem[inds]
            inst = _relabel_numpy(inst[inds], 'fill_gaps')
        down = self.preset['down']
        m, sf = self._augment_draws(rs)
        xyz_middle = np.matmul(xyz * sf if sf is not None else xyz, m)
        x = xyz_middle * self.scale / down if down != 1 else xyz_middle * self.scale
        if rs.rand() < self.aug_prob:
            if self.trace is not None:
                self.trace.append(('elastic', None, None))
            for gran, mag in ((6, 40.), (20, 160.)):
                bb = np.abs(x).max(0).astype(np.int32) // gran + 3
                grids = [blur_numpy(rs.grid_host(bb)) for _ in range(3)]
                x = x + np.stack([interp_numpy(gd, gran, x) for gd in grids], 1) * (mag / down if down != 1 else mag)
        if down != 1:
            x = x * down
        x = x - x.min(0)
        room = x.max(0) - x.min(0)

        def count(cands):
            out = []
            for o, ss in cands:
                xo = x + o
                if self.trace is not None:
                    self.trace.append(('crop', xo, ss))
                out.append(int(((xo.min(1) >= 0) * ((xo < ss).sum(1) == 3)).sum()))
            return out

        got = self._crop(rs, x.shape[0], room, count, spec=1)
        if got is None:
            return None
        off, shape, _ = got
        if off is None:
            keep = np.ones(x.shape[0], bool)
        else:
            x = x + off
            keep = (x.min(1) >= 0) * ((x < shape).sum(1) == 3)
        x, xyz_middle, rgb, sem = x[keep], xyz_middle[keep], rgb[keep], sem[keep]
        if self.trace is not None:
            self.trace.append(('coord', x, None))
        inst = _relabel_numpy(inst[keep], self.preset['relabel'])
        # getInstanceInfo (custom.py:76-90)
        lab = inst.astype(np.int32)
        n_inst = max(int(lab.max()) + 1, 0)
        pt_mean = np.ones((xyz_middle.shape[0], 3), dtype=np.float32) * -100.0
        pointnum, cls = [], []
        shift = self.preset['cls_shift']
        for i in range(n_inst):
            sel = np.where(lab == i)
            pt_mean[sel] = xyz_middle[sel].mean(0)
            pointnum.append(sel[0].size)
            c = sem[sel[0][0]]
            cls.append(c - shift if (shift and c != -100) else c)
        pt_offset = pt_mean - xyz_middle
        feat = torch.from_numpy(np.array(rgb, dtype=np.float32))
        feat += torch.from_numpy(np.asarray(rs.feat_noise(feat.size(1)), np.float32))
        return (torch.from_numpy(x).long(), torch.from_numpy(xyz_middle), feat, torch.from_numpy(sem),
                torch.from_numpy(inst), n_inst, pointnum, cls, torch.from_numpy(pt_offset))

    # ---- device --------------------------------------------------------------------------------------
    def _run_device(self, rs, xyz, rgb, sem, inst, words=None):
        return _DeviceRun(self, rs).run(xyz, rgb, sem, inst, words)


from ._train_device import _DeviceRun, collate_train_device  # noqa: E402,F401
