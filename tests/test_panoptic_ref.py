"""CPU side of the panoptic-fusion reference: tests/panoptic_ref.py against the two Python loops of the project
(SoftGroup.panoptic_fusion over RLE strings, the CPU oracle's over dense masks), its bit packing against a plain
loop, its constants against csrc/instances.hip, and -- in the manner of tests/test_conv_ref.py -- every case of
tests/test_panoptic_fusion_gpu.py against the conditions it was built to meet, on the reference alone: a
retuned constant or a generator that no longer reaches an order swap, a second scan trip or both sides of the
list boundary fails here, before anyone goes to a GPU."""
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import panoptic_ref as P  # noqa: E402
import test_panoptic_fusion_gpu as G  # noqa: E402

from oracle.model import OracleSoftGroup  # noqa: E402
from softgroup_amd.model.softgroup import SoftGroup  # noqa: E402
from softgroup_amd.util.rle import rle_encode  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'softgroup_amd', 'csrc', 'instances.hip')


@pytest.mark.parametrize('skip_iou', [0.5, 0.2, 0.0, 1.0])
def test_reference_equals_both_python_loops(skip_iou):
    rng = np.random.default_rng(11)
    n, n_inst = 3000, 30
    points_of = P.mixed_masks(rng, n, n_inst)[0]
    points_of[7] = np.zeros(0, np.int64)                       # an empty mask: RLE counts ''
    points_of[19] = points_of[3][:points_of[3].size // 2].copy()     # inside another one
    order = rng.permutation(n_inst)
    labels = P.labels_for(n_inst)
    sem = rng.integers(0, 19, n).astype(np.int64)
    conf = np.empty(n_inst)
    conf[order] = np.linspace(0.99, 0.01, n_inst)              # np.argsort(conf)[::-1] == order
    assert np.array_equal(np.argsort(conf)[::-1], order)
    preds = []
    for k in range(n_inst):
        mask = np.zeros(n, np.int32)
        mask[points_of[k]] = 1
        preds.append(dict(scan_id='s', label_id=int(labels[k]), conf=float(conf[k]), pred_mask=rle_encode(mask)))
    ref = P.panoptic_ref(points_of, order, labels, sem, n, 10, skip_iou, 19, 11)
    model = SimpleNamespace(semantic_classes=19, instance_classes=8, test_cfg=dict(panoptic_skip_iou=skip_iou))
    np.testing.assert_array_equal(ref.out, SoftGroup.panoptic_fusion(model, sem, preds))
    ora = SimpleNamespace(cfg=dict(semantic_classes=19, instance_classes=8, test_cfg=dict(panoptic_skip_iou=skip_iou)))
    np.testing.assert_array_equal(ref.out, OracleSoftGroup.panoptic_fusion(ora, sem, preds))
    # what it reports besides: decisions, ids, the one-hot statistics
    assert ref.out.dtype == np.uint32 and ref.pasted.shape == (n_inst,) and ref.stats.shape == (n_inst, 3)
    assert ref.n_ids == ref.pasted.sum() == ref.stats[:, :2].sum() and (ref.stats.sum(1) == 1).all()
    assert np.array_equal(ref.stats[:, P.SKIPPED] == 1, ~ref.pasted)
    ids = ref.out[ref.out != 19] >> 16
    assert set(ids[ids > 0].tolist()) <= set(range(1, ref.n_ids + 1))
    if skip_iou == 0.5:
        assert ref.stats.sum(0).min() > 0
        r7 = int(np.nonzero(order == 7)[0][0])                 # the empty mask is pasted and uses an id
        assert ref.pasted[r7] and not ((ref.out >> 16) == ref.pasted[:r7 + 1].sum()).any()
    if skip_iou == 0.0:
        assert ref.stats[:, P.PASTED_OVERLAP].sum() == 0
    if skip_iou == 1.0:
        assert ref.pasted.all() and ref.n_ids == n_inst


def test_pack_bits_equals_a_plain_loop():
    rng = np.random.default_rng(12)
    for n in (1, 31, 32, 33, 1000):
        points_of = P.mixed_masks(rng, n, 7)[0]
        points_of[2] = np.zeros(0, np.int64)
        bits = P.pack_bits(points_of, n)
        want = np.zeros((7, (n + 31) // 32), np.uint32)
        for k, pts in enumerate(points_of):
            for i in pts.tolist():
                want[k, i >> 5] |= np.uint32(1) << np.uint32(i & 31)
        assert bits.dtype == np.uint32
        np.testing.assert_array_equal(bits, want)
    assert P.pack_bits([], 100).shape == (0, 4) and P.pack_bits([np.zeros(0, np.int64)], 0).shape == (1, 0)
    with pytest.raises(AssertionError):
        P.pack_bits([np.array([3, 3])], 10)


def test_constants_are_those_of_the_kernel_source():
    src = open(SRC).read()

    def const(name):
        return re.search(r'constexpr int %s = ([^;]+);' % name, src).group(1)

    assert int(const('kFuseSumPerLane')) == 16 and const('kFuseTakenWords') == 'kFuseSumPerLane * 64 * 32'
    assert P.TAKEN_WORDS == 16 * 64 * 32 and int(const('kFuseListCap')) == P.LIST_CAP
    assert re.findall(r'SG_WALK\((\d+)\);', src) == ['1', '2', '4', '8', '16']
    assert 'const int spl = (sum_words + 63) / 64;' in src
    assert '__shared__ uint32_t pasted[2048];' in src and '(r & 63) == 63' in src
    assert 'n_inst) * sum_words * 32, 256, %d)' % (P.SUMMARY_CAP // 256) in src
    assert 'n_inst) * words, 256, %d)' % (P.ASSIGN_CAP // 256) in src
    assert P.ORDER_BLOCK == 64 and P.SCAN_TRIP == 2048
    assert [P.walk_width(n) for n in (1, 65536, 65537, 131072, 131073, 262144, 262145, 300000, 524288, 524289,
                                      1048576, 1048577)] == [1, 1, 2, 2, 4, 4, 8, 8, 8, 16, 16, None]


@pytest.mark.parametrize('case', G.ALL_CASES, ids=lambda c: '-'.join([c[0].__name__] + [str(a) for a in c[1:]]))
def test_every_gpu_case_meets_its_conditions_on_the_reference(case):
    c = case[0](*case[1:])
    G.conditions(c)
    # the conventions of every case, and nothing left out of the comparison
    assert c.bits.shape == (c.n_inst, P.words_of(c.n)) and c.bits.dtype == np.uint32
    assert np.array_equal(np.sort(c.order), np.arange(c.n_inst))
    assert c.n_inst < 2 or not np.array_equal(c.order, np.arange(c.n_inst))
    assert np.array_equal(c.labels, 1 + np.arange(c.n_inst) % 251)
    assert c.sem.min() >= 0 and c.sem.max() < 19 and c.ref.out.shape == (c.n,)
    popc = np.unpackbits(c.bits.view(np.uint8), axis=1).sum(1) if c.n_inst else np.zeros(0)
    assert np.array_equal(popc, [len(p) for p in c.points_of])
    if c.n % 32:
        assert (c.bits[:, -1] >> np.uint32(c.n % 32)).max() == 0, 'no bit behind the row'


def test_block_problems_reports_what_is_missing():
    one = np.eye(3, dtype=np.int64)
    st = np.stack([one[P.PASTED_FREE]] * 64 + [one[P.SKIPPED]] * 3)
    assert P.block_problems(st, 64) == [(0, 64, 64, 0)]
    st[10] = one[P.SKIPPED]
    assert P.block_problems(st, 64) == []
    assert P.block_problems(st[:64], 2048) == [] and P.block_problems(st[:5], 64) == [(0, 5, 5, 0)]
    assert P.block_problems(st[:1], 64) == []
    st8 = np.stack([one[P.PASTED_OVERLAP]] * 72)
    st8[3] = one[P.SKIPPED]
    assert P.block_problems(st8, 64) == [(64, 72, 8, 0)]
