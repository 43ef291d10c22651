"""Thinning a cloud before the network: the random sample of the reference's offline step
(dataset/s3dis/downsample.py: ``random.sample(range(N), int(N * ratio))``) and the voxel-grid downsample that
script leaves unimplemented (its ``--voxel-size`` branch raises).

``voxel_downsample`` keeps one point per occupied voxel and returns ``inverse``, the map from every original point
to its voxel's representative in the thinned cloud -- what ``softgroup_amd.util.propagate_result`` takes to carry a
result of the thinned cloud back.  The rules (cell = floor(float64(x) / voxel), representative, order) are those of
``softgroup_amd.ops.resample``.
"""
import random

import numpy as np

from ..ops import resample as RS

__all__ = ['voxel_downsample', 'random_downsample', 'apply_sample']


def voxel_downsample(xyz, voxel_size, pick='center', backend='auto'):
    """One point per occupied voxel -> (sample_ids, inverse): ``sample_ids`` ascending (the thinned cloud
    ``xyz[sample_ids]`` keeps the point order), ``inverse[i]`` = position in ``sample_ids`` of the representative of
    point i's voxel.  ``pick``: ``'center'`` the point nearest to the voxel's centre, ``'first'`` the lowest index.
    CUDA tensors in give CUDA int64 tensors out, numpy in gives numpy int64 out.  ``backend``: ``'device'`` (HIP
    kernels; numpy input is uploaded), ``'numpy'``, or ``'auto'`` (``ops.resample._AUTO``)."""
    import torch
    chosen = RS.auto_backend(backend, 'voxel')
    is_cuda = torch.is_tensor(xyz) and xyz.is_cuda
    if chosen == 'device':
        if not torch.cuda.is_available():
            raise RuntimeError("voxel_downsample: backend='device' without a GPU")
        d_xyz = xyz if is_cuda else RS._upload(RS._xyz_numpy(xyz))
        ids, inv = RS.grid_downsample(d_xyz, voxel_size, pick)
        ids, inv = ids.long(), inv.long()
        if is_cuda:
            return ids, inv
        ids, inv = ids.cpu(), inv.cpu()
        return (ids, inv) if torch.is_tensor(xyz) else (ids.numpy(), inv.numpy())
    ids, inv = RS.grid_downsample_numpy(xyz, voxel_size, pick)
    ids, inv = ids.astype(np.int64), inv.astype(np.int64)
    if torch.is_tensor(xyz):
        return torch.from_numpy(ids).to(xyz.device), torch.from_numpy(inv).to(xyz.device)
    return ids, inv


def random_downsample(n, ratio, seed=None, rng='python'):
    """``int(n * ratio)`` distinct indices below ``n``.  ``rng='python'``: ``random.Random(seed).sample(range(n),
    k)``, the reference's draw in the reference's unsorted order (numpy int64); ``rng='device'``: the first k of a
    seeded ``torch.randperm`` on the GPU (CUDA int64)."""
    n = int(n)
    k = int(n * ratio)
    if not 0 <= k <= n:
        raise ValueError(f'ratio {ratio!r}: between 0 and 1')
    if rng == 'python':
        return np.array(random.Random(seed).sample(range(n), k), dtype=np.int64)
    if rng == 'device':
        import torch
        gen = torch.Generator(device='cuda')
        if seed is None:
            gen.seed()
        else:
            gen.manual_seed(int(seed))
        return torch.randperm(n, generator=gen, device='cuda')[:k]
    raise ValueError(f"rng {rng!r}: one of 'python', 'device'")


def apply_sample(ids, xyz, rgb, semantic_label, instance_label):
    """the four gathers of the reference's ``random_sample``: -> (xyz, rgb, semantic_label, instance_label)[ids]"""
    import torch

    def take(a):
        if torch.is_tensor(a):
            return a[torch.as_tensor(ids, device=a.device).long()]
        return np.asarray(a)[ids.cpu().numpy() if torch.is_tensor(ids) else np.asarray(ids)]

    return take(xyz), take(rgb), take(semantic_label), take(instance_label)
