"""Several results over the SAME points combined into one (csrc/ensemble.hip): the per-point vote of the semantic
labels, the links between the instances of different passes over one stacked mask matrix, the objects those links
form and the per-point vote of every object's member masks.

The reference has none of these; the rules are this project's and are stated in include/softgroup_hip.h:

* K passes (1 <= K <= 32) over the same N points in the same order; pass p has an integer weight ``w_p >= 1``,
  ``W = sum w_p <= 32767``;
* label vote: at a point the label of pass p is COUNTED when it is ``>= 0`` and ``!= ignore_label``; ``count(c)`` is
  the sum of ``w_p`` over the passes that say c; the greatest count wins, the LOWEST class among equal counts; a
  point with no counted label keeps pass 0's value;
* links: instances are numbered g = 0 .. G-1 by (pass, list order); rows g < h are linked when they come from
  different passes, carry equal labels and ``ops.stitch.link_rule`` holds for their populations and intersection
  over all N points;
* an OBJECT is a connected component of the links, objects are ordered by their smallest member; the SUPPORT of an
  object is the sum of ``w_p`` over the distinct passes that have a member in it;
* mask vote: for object o and point x, v = the sum of ``w_p`` over the passes with at least one member of o that
  holds x (a pass counts once per point); the bit is set when ``v >= need[o]``.

All arithmetic is integer, apart from the one IEEE double division of the link rule.  CUDA tensors take the HIP
kernels, numpy arrays the ``*_numpy`` twins, which are the definition the device results are held to byte for byte.
"""
import numpy as np

from . import stitch as ST
from ._args import _words, choose_backend
from .nms import _measure, _popcount

__all__ = ['auto_backend', 'pass_weights', 'label_vote', 'label_vote_numpy', 'mask_group_links',
           'mask_group_links_numpy', 'objects_of_components', 'member_lists', 'mask_vote', 'mask_vote_numpy',
           'MAX_PASSES', 'MAX_WEIGHT', 'MAX_INSTANCES', 'MAX_DEVICE_POINTS']

MAX_PASSES = 32
MAX_WEIGHT = 32767
MAX_INSTANCES = ST.MAX_INSTANCES
MAX_DEVICE_POINTS = 2**31

# what backend='auto' means with a GPU present -- the single place to change.  Both follow
# profiles/ensemble_bench.txt, where the device is ahead of numpy on both clouds and for K = 4 and 8 (wall, MI355X,
# numpy arrays and RLE dicts in and out): the label vote 0.32 - 1.17 ms against 5.4 - 83.7 ms, the instances
# 3.3 - 28.3 ms against 198 - 4017 ms.
_AUTO = {'labels': 'device', 'instances': 'device'}


def auto_backend(backend, what):
    """'device' or 'numpy' for one of the operations of ``_AUTO``"""
    return choose_backend(backend, _AUTO[what])


def pass_weights(weights, k):
    """-> int64 [K]: the weights of K passes (``None``: all 1).  K outside 1 .. 32, a weight that is not an integer
    >= 1 or a sum above 32767 raises ``ValueError``."""
    k = int(k)
    if not 1 <= k <= MAX_PASSES:
        raise ValueError(f'{k} passes: between 1 and {MAX_PASSES}')
    if weights is None:
        return np.ones(k, np.int64)
    given = list(np.asarray(weights).reshape(-1).tolist()) if not isinstance(weights, (list, tuple)) else list(weights)
    if len(given) != k:
        raise ValueError(f'{len(given)} weights for {k} passes')
    out = np.empty(k, np.int64)
    for p, w in enumerate(given):
        if isinstance(w, (bool, np.bool_)) or not isinstance(w, (int, float, np.integer, np.floating)) or w != w \
                or w in (float('inf'), float('-inf')) or int(w) != w or int(w) < 1:
            raise ValueError(f'weight {w!r} of pass {p}: an integer >= 1')
        out[p] = int(w)
    if int(out.sum()) > MAX_WEIGHT:
        raise ValueError(f'weights that sum to {int(out.sum())}: at most {MAX_WEIGHT}')
    return out


# ---- label vote ------------------------------------------------------------------------------------------------------
def _label_rows(labels):
    labels = np.asarray(labels)
    if labels.ndim != 2 or labels.dtype.kind not in 'iu':
        raise ValueError('labels: an integer array [K, N]')
    return np.ascontiguousarray(labels, dtype=np.int64)


def label_vote_numpy(labels, weights=None, ignore_label=-100):
    """labels int64 [K, N] -> int64 [N]: the weighted vote per point.  Every pass's label is compared with every
    pass's (K ** 2 array comparisons); the first pass of the greatest count and, among equal counts, of the lowest
    class gives the value."""
    labels = _label_rows(labels)
    k, n = labels.shape
    weights = pass_weights(weights, k)
    ok = (labels >= 0) & (labels != int(ignore_label))
    best_c = np.zeros(n, np.int64)
    best_l = np.zeros(n, np.int64)
    for p in range(k):
        c = np.zeros(n, np.int64)
        for q in range(k):
            c += np.where(ok[q] & (labels[q] == labels[p]), weights[q], 0)
        better = ok[p] & ((c > best_c) | ((c == best_c) & (labels[p] < best_l)))
        best_c = np.where(better, c, best_c)
        best_l = np.where(better, labels[p], best_l)
    return np.where(best_c > 0, best_l, labels[0])


def label_vote(labels, weights=None, ignore_label=-100):
    """``sg_label_vote`` on a CUDA int64 tensor [K, N] -> CUDA int64 [N].  Nothing synchronises.  Other inputs:
    numpy."""
    import torch
    if not (torch.is_tensor(labels) and labels.is_cuda):
        return label_vote_numpy(labels.numpy() if torch.is_tensor(labels) else labels, weights, ignore_label)
    from .. import _lib as L
    if labels.dim() != 2 or labels.is_floating_point():
        raise ValueError('labels: an integer tensor [K, N]')
    k, n = labels.size(0), labels.size(1)
    w = pass_weights(weights, k)
    if n >= MAX_DEVICE_POINTS:
        raise L.SoftGroupHipError(f'label_vote: {n} points: outside the supported range (n < 2**31)')
    labels = labels.to(torch.int64).contiguous()
    dev = labels.device
    with torch.cuda.device(dev):
        d_w = torch.from_numpy(w.astype(np.int32)).to(dev)
        out = torch.empty(n, dtype=torch.int64, device=dev)
        L.check(L.lib().sg_label_vote(L.ptr(labels) if n else None, k, n, L.ptr(d_w), int(ignore_label),
                                      L.ptr(out) if n else None, L.stream()), 'sg_label_vote')
    return out


# ---- links -----------------------------------------------------------------------------------------------------------
def _rows8(bits, n):
    """packed rows of any integer dtype -> uint8 [n, bytes per row]"""
    bits = np.ascontiguousarray(bits)
    return bits.view(np.uint8).reshape(n, -1) if n and bits.size else np.zeros((n, 0), np.uint8)


def mask_group_links_numpy(bits, n_bits, labels, group, thr=0.5, measure='iou', min_shared=1):
    """packed rows [G, >= ceil(n_bits / 8) bytes], labels [G], group [G] -> the symmetric adjacency uint32
    [G, ceil(G / 32)] that ``stitch_components`` takes: rows g < h of different groups and equal labels, decided by
    ``ops.stitch.link_rule`` on their populations and intersection over the n_bits points"""
    _measure(measure)
    labels, group = np.asarray(labels).reshape(-1), np.asarray(group).reshape(-1)
    g_total = labels.size
    if group.size != g_total or np.asarray(bits).shape[0] != g_total:
        raise ValueError('labels, group: one entry per row')
    adj = np.zeros((g_total, _words(g_total)), dtype=np.uint32)
    if g_total == 0:
        return adj
    rows = ST._rows64(_rows8(bits, g_total), n_bits)
    cnt = _popcount(rows).sum(1, dtype=np.int64) if rows.size else np.zeros(g_total, np.int64)
    idx = np.arange(g_total)
    for g in range(g_total):
        cand = np.flatnonzero((idx > g) & (group != group[g]) & (labels == labels[g]))
        if cand.size == 0:
            continue
        inter = _popcount(rows[cand] & rows[g]).sum(1, dtype=np.int64) if rows.size else np.zeros(cand.size, np.int64)
        for h in cand[ST.link_rule(inter, cnt[g], cnt[cand], thr, measure, min_shared)].tolist():
            adj[g, h >> 5] |= np.uint32(1 << (h & 31))
            adj[h, g >> 5] |= np.uint32(1 << (g & 31))
    return adj


def _bit_rows(bits, n_bits):
    if bits.dim() != 2 or bits.element_size() != 4 or bits.is_floating_point() or bits.size(1) != _words(n_bits):
        raise ValueError(f'bits: an integer tensor [n, {_words(n_bits)}] of 32-bit words')
    return bits.contiguous()


def mask_group_links(bits, n_bits, labels, group, thr=0.5, measure='iou', min_shared=1):
    """``sg_mask_group_links`` on CUDA bit rows int32 [G, ceil(n_bits / 32)] -> adj int32 [G, ceil(G / 32)] on the
    device.  Nothing synchronises.  Other inputs: numpy."""
    import torch
    if not (torch.is_tensor(bits) and bits.is_cuda):
        return mask_group_links_numpy(bits.numpy() if torch.is_tensor(bits) else bits, n_bits, labels, group, thr,
                                      measure, min_shared)
    from .. import _lib as L
    meas = _measure(measure)
    n_bits = int(n_bits)
    bits = _bit_rows(bits, n_bits)
    dev, g_total = bits.device, bits.size(0)
    if g_total > MAX_INSTANCES or n_bits >= MAX_DEVICE_POINTS:
        raise L.SoftGroupHipError(f'mask_group_links: {g_total} instances over {n_bits} points: outside the supported '
                                  f'range (at most {MAX_INSTANCES}, fewer than 2**31)')
    labels = torch.as_tensor(labels).to(dev, torch.int32).reshape(-1).contiguous()
    group = torch.as_tensor(group).to(dev, torch.int32).reshape(-1).contiguous()
    if labels.numel() != g_total or group.numel() != g_total:
        raise ValueError('labels, group: one entry per row')
    with torch.cuda.device(dev):
        adj = torch.zeros((g_total, _words(g_total)), dtype=torch.int32, device=dev)
        L.check(L.lib().sg_mask_group_links(L.ptr(bits) if bits.numel() else None, g_total, n_bits,
                                            L.ptr(labels) if g_total else None, L.ptr(group) if g_total else None,
                                            float(thr), meas, int(min_shared), L.ptr(adj) if g_total else None,
                                            L.stream()), 'sg_mask_group_links')
    return adj


# ---- objects ---------------------------------------------------------------------------------------------------------
def objects_of_components(comp, group, weights):
    """``comp`` (the smallest member of every instance's component), the pass of every instance and the pass
    weights -> (objects: the member lists, ascending, in ascending order of their smallest member; support int64
    [n_obj]: the sum of w_p over the distinct passes with a member).  O(G) on the host."""
    members = {}
    for g, root in enumerate(np.asarray(comp).reshape(-1).tolist()):
        members.setdefault(int(root), []).append(g)
    objects = [members[root] for root in sorted(members)]
    group, weights = np.asarray(group).reshape(-1), np.asarray(weights).reshape(-1)
    support = np.array([int(weights[np.unique(group[m])].sum()) for m in objects], dtype=np.int64).reshape(-1)
    return objects, support


def member_lists(objects, group, weights):
    """member lists -> what ``sg_mask_vote`` takes: (obj_off int32 [n_obj + 1], members, member_weight, member_pass
    int32), the members of an object sorted by (pass, instance)"""
    group, weights = np.asarray(group).reshape(-1), np.asarray(weights).reshape(-1)
    obj_off = np.zeros(len(objects) + 1, np.int32)
    members = []
    for o, m in enumerate(objects):
        members += sorted(m, key=lambda g: (int(group[g]), g))
        obj_off[o + 1] = len(members)
    members = np.array(members, dtype=np.int32).reshape(-1)
    passes = group[members].astype(np.int32)
    return obj_off, members, weights[passes].astype(np.int32), passes


# ---- mask vote -------------------------------------------------------------------------------------------------------
def mask_vote_numpy(bits, n_bits, obj_of, group, weights, need):
    """packed rows [G, ...], obj_of [G] (-1: in no object), group [G], weights [K], need [n_obj] (>= 1) -> (rows
    uint32 [n_obj, ceil(n_bits / 32)], npoint int32 [n_obj]): per object and point the weights of the passes that
    hold the point are added up (a pass once per point) and compared with ``need``"""
    n_bits = int(n_bits)
    obj_of, group = np.asarray(obj_of).reshape(-1), np.asarray(group).reshape(-1)
    weights, need = np.asarray(weights).reshape(-1), np.asarray(need).reshape(-1)
    g_total, n_obj, k = obj_of.size, need.size, weights.size
    pass_weights(weights.tolist(), k)
    if group.size != g_total or np.asarray(bits).shape[0] != g_total:
        raise ValueError('obj_of, group: one entry per row')
    if n_obj and int(need.min()) < 1:
        raise ValueError('need: at least 1')
    if g_total and (int(obj_of.max()) >= n_obj or int(group.min()) < 0 or int(group.max()) >= k):
        raise ValueError('obj_of / group: an object or a pass that does not exist')
    words = _words(n_bits)
    out = np.zeros((n_obj, words * 4), dtype=np.uint8)
    npoint = np.zeros(n_obj, np.int32)
    rows = _rows8(bits, g_total)
    nbytes = (n_bits + 7) // 8
    if n_obj == 0 or n_bits == 0 or g_total == 0:
        return out.view(np.uint32).reshape(n_obj, words), npoint
    order = np.lexsort((group, obj_of))                             # by (object, pass), stable
    order = order[obj_of[order] >= 0]
    starts = np.searchsorted(obj_of[order], np.arange(n_obj + 1))
    for o in range(n_obj):
        mem = order[starts[o]:starts[o + 1]]
        v = np.zeros(n_bits, np.int64)
        for p in np.unique(group[mem]).tolist():
            held = np.bitwise_or.reduce(rows[mem[group[mem] == p], :nbytes], axis=0)
            v += int(weights[p]) * np.unpackbits(held, bitorder='little')[:n_bits].astype(np.int64)
        hit = v >= int(need[o])
        npoint[o] = int(hit.sum())
        out[o, :nbytes] = np.packbits(hit, bitorder='little')
    return out.view(np.uint32).reshape(n_obj, words), npoint


def mask_vote(bits, n_bits, obj_off, members, member_weight, member_pass, need):
    """``sg_mask_vote`` on CUDA bit rows int32 [G, ceil(n_bits / 32)] and the lists of ``member_lists`` (host or
    device; handed on as they are -- the kernel ignores an entry outside its range) -> (out_bits int32
    [n_obj, ceil(n_bits / 32)], npoint int32 [n_obj]) on the device.  Nothing synchronises."""
    import torch

    from .. import _lib as L
    n_bits = int(n_bits)
    bits = _bit_rows(bits, n_bits)
    dev, g_total = bits.device, bits.size(0)

    def i32(a):
        return torch.as_tensor(a).to(dev, torch.int32).reshape(-1).contiguous()

    obj_off, need = i32(obj_off), i32(need)
    n_obj = need.numel()
    if obj_off.numel() != n_obj + 1:
        raise ValueError('obj_off: one entry per object and one more')
    if g_total > MAX_INSTANCES or n_obj > MAX_INSTANCES or n_bits >= MAX_DEVICE_POINTS:
        raise L.SoftGroupHipError(f'mask_vote: {g_total} instances, {n_obj} objects over {n_bits} points: outside the '
                                  f'supported range (at most {MAX_INSTANCES}, fewer than 2**31)')
    lists = []
    for a in (members, member_weight, member_pass):
        a = i32(a)
        if a.numel() > g_total:
            raise ValueError('members: at most one entry per row of bits')
        full = torch.full((max(g_total, 1), ), -1, dtype=torch.int32, device=dev)   # (the unused tail: ignored entries)
        full[:a.numel()] = a
        lists.append(full)
    with torch.cuda.device(dev):
        out_bits = torch.empty((n_obj, _words(n_bits)), dtype=torch.int32, device=dev)
        npoint = torch.zeros(n_obj, dtype=torch.int32, device=dev)
        L.check(L.lib().sg_mask_vote(L.ptr(bits) if bits.numel() else None, g_total, n_bits, L.ptr(obj_off),
                                     L.ptr(lists[0]), L.ptr(lists[1]), L.ptr(lists[2]), L.ptr(need) if n_obj else None,
                                     n_obj, L.ptr(out_bits) if out_bits.numel() else None,
                                     L.ptr(npoint) if n_obj else None, L.stream()), 'sg_mask_vote')
    return out_bits, npoint
