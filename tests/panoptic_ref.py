"""Host reference of the panoptic fusion (csrc/instances.hip, sg_panoptic_fusion), exactly as the reference
model states it (softgroup.py:606-639):

    for every instance in the given order:
        overlap = points of the instance that an earlier instance took
        if overlap / (size + 1e-5) > skip_iou:  skip it                      (float64)
        otherwise its FREE points get the instance's class and the next id; next id += 1
    out = class | id << 16; a point with a thing class and no id becomes `semantic_classes`

Test helper.  Nothing here touches the HIP library.  ``panoptic_ref`` works over per-instance sorted index
arrays, never over dense N-vectors per instance, so that a million-point row with 70 instances or 65 535
instances of a few points each cost what their points cost.  tests/test_panoptic_ref.py pins it to the two
Python loops of the project (SoftGroup.panoptic_fusion over RLE strings, the CPU oracle's over dense masks).

Besides the output it returns what a test needs to know that a case reaches what it was built for: the
paste / skip decision per visiting rank, the number of ids handed out and, per rank, a one-hot count of
{pasted with no overlap, pasted with overlap, skipped} -- ``stats[a:b].sum(0)`` counts a range of ranks.

The case generators of tests/test_panoptic_fusion_gpu.py live here as well, so that the conditions the cases
have to meet (a paste and a skip in every 64-rank order block and every 2048-rank scan trip, ...) are
checked on the reference alone, without a GPU, by tests/test_panoptic_ref.py.
"""
from collections import namedtuple

import numpy as np

PASTED_FREE, PASTED_OVERLAP, SKIPPED = 0, 1, 2

Fusion = namedtuple('Fusion', 'out pasted n_ids stats')

# the conventions of every case: the KITTI configuration of the model
CLS_OFFSET, SEMANTIC_CLASSES, THING_CLASS_MIN = 10, 19, 11

# constants of the walker (csrc/instances.hip); tests/test_panoptic_ref.py reads them back from the source
TAKEN_WORDS = 32768         # kFuseTakenWords: longer rows take the dense kernel
LIST_CAP = 8192             # kFuseListCap: more non-zero words are walked per lane, not from the LDS list
ORDER_BLOCK = 64            # ranks per register of the visiting order
SCAN_TRIP = 64 * 32         # ranks per trip of the decisions-to-ids scan (64 lanes x 32 bits of `pasted`)
SUMMARY_CAP = 4096 * 256    # threads of panoptic_summary_kernel at its block cap
ASSIGN_CAP = 8192 * 256     # threads of panoptic_assign_kernel at its block cap


def words_of(n):
    return (n + 31) // 32


def summary_words_of(n):
    return (words_of(n) + 31) // 32


def walk_width(n):
    """the instantiation of panoptic_walk_kernel<SPL> that a row of n points takes: the smallest of 1, 2, 4,
    8, 16 that holds ceil(ceil(ceil(n / 32) / 32) / 64) summary words per lane"""
    need = (summary_words_of(n) + 63) // 64
    return next((s for s in (1, 2, 4, 8, 16) if need <= s), None)      # None: the row takes the dense kernel


def panoptic_ref(points_of, order, labels, sem, n, cls_offset, skip_iou, semantic_classes, thing_class_min):
    """points_of[k]: sorted int64 point indices of instance k; order[r]: the instance visited at rank r"""
    sem = np.asarray(sem)
    assert sem.shape == (n,)
    cls = sem.astype(np.uint32)
    ids = np.zeros(n, np.uint32)
    taken = np.zeros(n, bool)
    n_rank = len(order)
    pasted = np.zeros(n_rank, bool)
    stats = np.zeros((n_rank, 3), np.int64)
    skip_iou = float(skip_iou)
    next_id = 1
    for r in range(n_rank):
        k = int(order[r])
        pts = points_of[k]
        hit = taken[pts]
        overlap = int(np.count_nonzero(hit))
        if float(overlap) / (float(pts.size) + 1e-5) > skip_iou:      # IEEE double, as numpy evaluates it
            stats[r, SKIPPED] = 1
            continue
        paste = pts[~hit]
        cls[paste] = np.uint32(int(labels[k]) + cls_offset)
        ids[paste] = next_id
        taken[paste] = True
        pasted[r] = True
        stats[r, PASTED_OVERLAP if overlap else PASTED_FREE] = 1
        next_id += 1          # also for an empty or a fully taken instance: it was pasted
    out = (cls & np.uint32(0xFFFF)) | (ids << np.uint32(16))
    out[(cls >= thing_class_min) & (ids == 0)] = semantic_classes
    return Fusion(out.astype(np.uint32), pasted, next_id - 1, stats)


def pack_bits(points_of, n):
    """uint32 [n_inst, ceil(n / 32)]: bit (p & 31) of word (p >> 5) of row k for every p in points_of[k]"""
    n_inst, words = len(points_of), words_of(n)
    if n_inst == 0 or words == 0:
        return np.zeros((n_inst, words), np.uint32)
    sizes = np.array([len(p) for p in points_of], np.int64)
    pts = np.concatenate([np.asarray(p, np.int64) for p in points_of]) if sizes.sum() else np.zeros(0, np.int64)
    inst = np.repeat(np.arange(n_inst, dtype=np.int64), sizes)
    assert pts.size == 0 or (pts.min() >= 0 and pts.max() < n)
    key = inst * n + pts
    assert np.all(np.diff(key) > 0), 'every instance: sorted, no point twice'
    # every (row, word, bit) occurs once, so the sum of the bit values is their OR; < 2^32: exact in float64
    flat = np.bincount(inst * words + (pts >> 5), weights=np.ldexp(1.0, (pts & 31).astype(np.int32)),
                       minlength=n_inst * words)
    return flat.astype(np.uint64).astype(np.uint32).reshape(n_inst, words)


def labels_for(n_inst):
    return (1 + np.arange(n_inst) % 251).astype(np.int32)


def block_problems(stats, block):
    """the condition on a case: every `block` ranks hold a pasted and a skipped instance; a trailing group of
    fewer than 8 ranks holds at least one of either; the case as a whole holds both (a case of one instance
    cannot: nothing is taken when its only instance is visited, so it is pasted)"""
    n_rank = len(stats)
    p = stats[:, PASTED_FREE] + stats[:, PASTED_OVERLAP]
    s = stats[:, SKIPPED]
    assert np.all(p + s == 1), 'every rank decided once'
    bad = []
    for lo in range(0, n_rank, block):
        hi = min(n_rank, lo + block)
        np_, ns_ = int(p[lo:hi].sum()), int(s[lo:hi].sum())
        if hi - lo < 8:
            ok = np_ + ns_ >= 1
        else:
            ok = np_ >= 1 and ns_ >= 1
        if not ok:
            bad.append((lo, hi, np_, ns_))
    if n_rank >= 2 and not (p.sum() >= 1 and s.sum() >= 1):
        bad.append((0, n_rank, int(p.sum()), int(s.sum())))
    return bad


# ---------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------
RUN, SCATTER, COPY, ENDS, TAIL = range(5)


def mixed_masks(rng, n, n_inst, order=None, size=None):
    """n_inst masks over n points, a mix of five shapes.  Returns points_of, `kinds` and, for the copies,
    `copy_of[k] = (instance copied, 65 536-point stretch copied from)`:
      RUN      a contiguous run with 20 % holes inside one aligned 1024-point group: all its words fall under
               ONE lane's summary word;
      SCATTER  points all over the row, one at least in every 65 536-point stretch: non-zero words under many
               lanes and under every summary word j of a lane;
      COPY     a near copy of an earlier instance, so that which of the two is pasted depends on the order:
               85 % of what that instance has inside ONE stretch and 0.6 times as many fresh points in the
               next stretch.  With `order` the copied instance is one that is visited earlier: the copy is
               skipped for an overlap of at least 0.62 that lies in that stretch alone.  The walker only hands
               on decisions (the ids come from the bit rows), so a stretch -- the summary word j of every
               lane -- that it reads wrongly shows ONLY where a decision hangs on it.  The copies go round
               the stretches; there are at least two more of them than stretches;
      ENDS     points of the row's first and of its last word only;
      TAIL     a holed run that ends on the row's last point, bit (n - 1) & 31 of the last word."""
    words = words_of(n)
    if size is None:
        size = int(max(3, min(400, 3 * n // (2 * max(n_inst, 1)))))
    n_groups = (n + 1023) // 1024
    n_stretch = (n + 65535) // 65536
    run_groups = rng.choice(n_groups, size=min(n_groups, max(1, n_inst // 8)), replace=False)
    if n_inst > 5:
        n_copy = max(n_inst // 5, min(n_stretch + 2, n_inst // 3))
        rest = np.array([RUN, SCATTER, ENDS, TAIL])[np.arange(n_inst - n_copy) % 4]
        kinds = np.concatenate([np.full(n_copy, COPY), rest])[rng.permutation(n_inst)]
    else:
        kinds = (np.arange(n_inst) + 4) % 5          # (a single instance is a TAIL: the row's last bit)
    rank_of = np.empty(n_inst, np.int64)
    rank_of[np.arange(n_inst) if order is None else np.asarray(order)] = np.arange(n_inst)
    points_of = [None] * n_inst
    for k in range(n_inst):
        kind = int(kinds[k])
        if kind == RUN:
            g = int(rng.choice(run_groups))
            lo, hi = g * 1024, min(n, g * 1024 + 1024)
            length = int(min(hi - lo, rng.integers(max(1, size // 2), 2 * size + 1)))
            a = int(rng.integers(lo, hi - length + 1))
            pts = np.arange(a, a + length)
            keep = rng.random(length) < 0.8
            keep[int(rng.integers(0, length))] = True
            pts = pts[keep]
        elif kind == SCATTER:
            forced = [int(rng.integers(lo, min(n, lo + 65536))) for lo in range(0, n, 65536)]
            pts = np.unique(np.concatenate([rng.integers(0, n, 2 * size), np.array(forced, np.int64)]))
        elif kind == ENDS:
            first = np.arange(0, min(32, n))
            last = np.arange(32 * (words - 1), n)
            f = first[rng.random(first.size) < 0.6]
            la = last[rng.random(last.size) < 0.6]
            pts = np.unique(np.concatenate([f, la, [int(rng.choice(first))], [int(rng.choice(last))]]))
        elif kind == TAIL:
            length = int(min(n, rng.integers(max(1, size // 2), 2 * size + 1)))
            pts = np.arange(n - length, n)
            keep = rng.random(length) < 0.8
            keep[-1] = True
            pts = pts[keep]
        else:
            continue
        points_of[k] = np.ascontiguousarray(pts, dtype=np.int64)
    # the copies, latest visited first: those have the widest choice of instances visited before them
    copy_of = {}
    copies = sorted((k for k in range(n_inst) if kinds[k] == COPY), key=lambda k: -rank_of[k])
    for i, k in enumerate(copies):
        g = i % n_stretch
        src = [j for j in range(n_inst) if kinds[j] in (RUN, SCATTER, TAIL)]
        for want in (lambda j: rank_of[j] < rank_of[k] and ((points_of[j] >> 16) == g).sum() >= 1 and
                     (kinds[j] == SCATTER or n_stretch == 1),
                     lambda j: rank_of[j] < rank_of[k], lambda j: True):
            cand = [j for j in src if want(j)]
            if cand:
                break
        if not cand:                                 # (nothing to copy: fewer than three instances)
            kinds[k] = RUN
            points_of[k] = np.arange(0, min(n, size), dtype=np.int64)
            continue
        j = int(rng.choice(cand))
        base = points_of[j]
        if not ((base >> 16) == g).any():
            g = int(rng.choice(base >> 16))
        inside = base[(base >> 16) == g]
        keep = rng.random(inside.size) < 0.85
        keep[int(rng.integers(0, inside.size))] = True
        h = (g + 1) % n_stretch
        if n - h * 65536 < 1024:                     # (a last stretch of a point or two has no room)
            h = (h + 1) % n_stretch
        fresh = rng.integers(h * 65536, min(n, h * 65536 + 65536), int(0.6 * keep.sum()))
        points_of[k] = np.unique(np.concatenate([inside[keep], fresh])).astype(np.int64)
        copy_of[k] = (j, g)
    return points_of, kinds, copy_of


def id_scan_masks(n_inst):
    """n = 3 n_inst: instance k owns [3k, 3k + 3); every third one also holds the points of k - 1 (visited
    first it takes them and k - 1 is skipped; visited second it is pasted with overlap 3 / 6); every seventh
    one is an exact copy of the instance before it (whichever of the two comes later is skipped)"""
    points_of = []
    for k in range(n_inst):
        if k >= 7 and k % 7 == 0:
            pts = points_of[k - 1].copy()
        elif k >= 3 and k % 3 == 0:
            pts = np.arange(3 * k - 3, 3 * k + 3)
        else:
            pts = np.arange(3 * k, 3 * k + 3)
        points_of.append(pts.astype(np.int64))
    return points_of


def many_instance_masks(rng, order, n=2048, free=960):
    """one mask per rank of `order` (65 535 of them on 2048 points): clusters of four points inside
    [0, free), which fill up within a few hundred ranks, after which such an instance is skipped.  So that
    every 64-rank order block still pastes and skips: rank 64 b + 5 is an exact copy of rank 64 b + 4
    (skipped), rank 64 b + 40 holds the reserved point free + b, which nobody else has, and one point of the
    crowd (overlap <= 1 / 2: pasted), and rank 64 b + 20 of every 16th block is an empty mask (pasted)."""
    n_inst = len(order)
    assert free + (n_inst + 63) // 64 <= n
    start = rng.integers(0, free - 10, n_inst)
    gaps = np.cumsum(rng.integers(1, 4, (n_inst, 3)), axis=1)
    crowd = np.concatenate([start[:, None], start[:, None] + gaps], axis=1).astype(np.int64)
    by_rank = [crowd[r] for r in range(n_inst)]
    for r in range(n_inst):
        b, i = divmod(r, 64)
        if i == 5:
            by_rank[r] = by_rank[r - 1].copy()
        elif i == 40:
            by_rank[r] = np.array([crowd[r, 0], free + b], np.int64)
        elif i == 20 and b % 16 == 0:
            by_rank[r] = np.zeros(0, np.int64)
    points_of = [None] * n_inst
    for r in range(n_inst):
        points_of[int(order[r])] = by_rank[r]
    return points_of


def list_boundary_masks(rng, n=300000):
    """the three large instances of the list-boundary case and eleven ordinary ones.  Returns points_of and
    the indices by name: X has exactly LIST_CAP non-zero words (one bit in each: the last row the LDS list
    takes), Y has LIST_CAP + 1 (the first row walked per lane), Z holds every point.  The walker's `taken` row
    is seen only through later decisions, so the large rows are probed by small instances that are free
    unless X (Y) was pasted word for word.  X's words are taken in the order of the walker's list (lane l's
    words behind those of the lanes before it; lane l owns the summary words l, l + 64, ...): x_first and
    x_last hold the ONE point of list entry 0 and of entry LIST_CAP - 1, x_head and x_tail those of the 40
    entries next to them.  Y's are taken by word: y_first / y_last the point of its lowest and of its highest
    word, y_head / y_tail those of the 40 words next to them.  r0 .. r2 are ordinary masks of the mix above."""
    words = words_of(n)
    assert words > LIST_CAP + 1 and n % 32 == 0

    def one_bit_per_word(count):
        w = np.sort(rng.choice(words, count, replace=False)).astype(np.int64)
        return w * 32 + rng.integers(0, 32, count)

    x, y = one_bit_per_word(LIST_CAP), one_bit_per_word(LIST_CAP + 1)
    summary_word = x >> 10
    x = x[np.lexsort((x, summary_word >> 6, summary_word & 63))]          # by lane, then j, then word
    ordinary = mixed_masks(rng, n, 3)[0]
    masks = dict(X=x, Y=y, Z=np.arange(n, dtype=np.int64), x_head=x[1:41], x_tail=x[-41:-1], y_head=y[1:41],
                 y_tail=y[-41:-1], x_first=x[:1], x_last=x[-1:], y_first=y[:1], y_last=y[-1:],
                 **{f'r{i}': ordinary[i] for i in range(3)})
    names = list(masks)
    slot = rng.permutation(len(names))
    points_of = [None] * len(names)
    index = {}
    for name, s in zip(names, slot):
        points_of[int(s)] = np.sort(masks[name]).astype(np.int64)
        index[name] = int(s)
    return points_of, index


def threshold_masks(ti=37, tc=111):
    """hand-made: A and B are pasted whole; C has tc points of which ti are theirs; D is an all-zero row;
    E is free and visited right after D (its id shows that D consumed one); F lies inside A (fully taken);
    G has one point of B and nine free ones.  Visited in this order: A B C D E F G."""
    assert 1 <= ti <= 60 and ti <= tc <= ti + 90
    from_a = min(ti, 20)
    masks = dict(A=np.arange(0, 50), B=np.arange(100, 150),
                 C=np.concatenate([np.arange(50 - from_a, 50), np.arange(100, 100 + ti - from_a),
                                   np.arange(200, 200 + tc - ti)]),
                 D=np.zeros(0, np.int64), E=np.arange(300, 320), F=np.arange(5, 25),
                 G=np.concatenate([[149], np.arange(330, 339)]))
    assert masks['C'].size == tc
    names = list('ABCDEFG')
    slot = [4, 0, 6, 2, 5, 1, 3]                 # where each mask is stored: the order is no identity
    points_of = [None] * 7
    for name, s in zip(names, slot):
        points_of[s] = np.ascontiguousarray(masks[name], dtype=np.int64)
    return points_of, np.array(slot, np.int32), names
