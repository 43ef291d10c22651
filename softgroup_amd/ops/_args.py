"""The small argument helpers the ops modules share: the backend rule, arrays to and from the device, the checks of
an ``xyz`` argument.  Private: the modules import what they use under the same names."""
import numpy as np


def choose_backend(backend, auto):
    """'device' or 'numpy': ``auto`` (the caller's ``_AUTO`` entry, read when it calls) for ``'auto'`` with a GPU
    present, numpy for ``'auto'`` without one, an explicit backend as given"""
    if backend not in ('auto', 'device', 'numpy'):
        raise ValueError(f"backend {backend!r}: one of 'auto', 'device', 'numpy'")
    if backend == 'auto':
        import torch
        backend = auto if torch.cuda.is_available() else 'numpy'
    return backend


def _host(a):
    import torch
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _is_cuda(a):
    import torch
    return torch.is_tensor(a) and a.is_cuda


def _upload(a):
    """CUDA tensor of a host array (a read-only array is copied first: torch cannot wrap one)"""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()


def _xyz_numpy(xyz, what='xyz'):
    xyz = np.ascontiguousarray(_host(xyz), dtype=np.float32)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError(f'{what}: an array [n, 3]')
    return xyz


def _xyz_device(xyz, what='xyz'):
    import torch
    if xyz.dim() != 2 or xyz.size(1) != 3:
        raise ValueError(f'{what}: a tensor [n, 3]')
    if xyz.size(0) >= 2**31:
        raise ValueError(f'{what}: fewer than 2**31 points')
    return xyz.detach().to(torch.float32).contiguous()


def _max_dist(max_dist):
    if max_dist is None:
        return -1.0
    max_dist = float(max_dist)
    if not max_dist >= 0.0:
        raise ValueError(f'max_dist {max_dist!r}: None or a number >= 0')
    return max_dist


def _words(n):
    return (int(n) + 31) // 32
