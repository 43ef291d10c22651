"""Keeps the sizes of tests/test_launch_caps_gpu.py honest: the launch caps are derived here from the sources (one
regular expression each), and every size the GPU tests use must sit on the side of its cap it was chosen for.  When a
grid or a block is retuned this test names the sizes to move, instead of the GPU tests quietly making one trip through
every loop again."""
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import torch  # noqa: E402

_GPU_UP_BEFORE = torch.cuda.is_initialized()
import test_launch_caps_gpu as G  # noqa: E402

_GPU_UP_AFTER = torch.cuda.is_initialized()

PKG = os.path.join(os.path.dirname(HERE), 'softgroup_amd')


def _src(*path):
    with open(os.path.join(*path)) as f:
        return f.read()


def _csrc(name):
    return _src(PKG, 'csrc', name)


def _const(src, name):
    m = re.search(r'constexpr\s+int\s+' + name + r'\s*=\s*(\d+)\s*;', src)
    assert m, f'constexpr int {name} not found'
    return int(m.group(1))


def _launch_cap(src, kernel, items):
    """block * max_blocks of `kernel<<<grid_for(items, block, max_blocks), ...`"""
    m = re.search(kernel + r'<<<\s*grid_for\(\s*' + items + r'\s*,\s*(\w+)\s*,\s*(\d+)\s*\)\s*,\s*(\w+)\s*,', src)
    assert m, f'the launch of {kernel} not found'
    assert m.group(1) == m.group(3), (kernel, m.groups())                 # grid and launch use the same block
    block = int(m.group(1)) if m.group(1).isdigit() else _const(src, m.group(1))
    return block * int(m.group(2))


def test_importing_the_gpu_module_does_not_touch_the_gpu():
    assert _GPU_UP_BEFORE or not _GPU_UP_AFTER
    assert G.pytestmark.name == 'gpu'


def test_tally_sizes_sit_on_both_sides_of_the_grid_cap():
    s = _csrc('eval_ops.hip')
    assert re.search(r'tally_grid\(int64_t n\)\s*\{\s*return grid_for\(\(n \+ 3\) / 4, kTallyBlock, kTallyMaxGrid\);', s)
    cap = _const(s, 'kTallyBlock') * _const(s, 'kTallyMaxGrid') * 4
    assert cap == G.TALLY_CAP == 1048576
    sizes = [n for n, _ in G.TALLY_CASES]
    assert cap in sizes and cap + 1 in sizes                                  # the last one-trip size, the first above
    assert any(n > cap and n % 4 == 3 for n in sizes)                         # a scalar tail in the second trip
    assert any(n > 2 * cap and n % 4 for n in sizes)                          # a third trip
    assert {dt for n, dt in G.TALLY_CASES if n > cap} == {'int32', 'int64'}
    from softgroup_amd.evaluation import point_wise_eval as pw
    assert max(sizes) <= pw._CHUNK_POINTS                                     # one chunk = one launch
    # where the older tests stop: 4 x 150 000 points (point-wise), 8 x 120 000 (PanopticEval), both in one chunk
    old = _src(HERE, 'test_pointwise_eval_gpu.py')
    m = re.search(r'pc\.scannet_like\(200 \+ s, (\d+)\) for s in range\((\d+)\)', old)
    assert m and int(m.group(1)) * int(m.group(2)) == 600000 < cap
    m = re.search(r'pc\.kitti_like\(100 \+ s, (\d+)\) for s in range\((\d+)\)', old)
    assert m and int(m.group(1)) * int(m.group(2)) == 960000 < cap


def test_panoptic_set_is_one_chunk_above_the_insert_cap():
    s = _csrc('eval_ops.hip')
    cap = _launch_cap(s, 'pan_insert_kernel', 'n_points')
    assert cap == G.PAN_CAP == 4096 * 256
    total = G.PAN_SCANS * G.PAN_SCAN_POINTS
    m = re.search(r'max_chunk_points=(\d+) << (\d+)', _src(PKG, 'evaluation', 'panoptic_eval.py'))
    assert m and cap < total <= int(m.group(1)) << int(m.group(2))
    # PanopticEval runs the tally with panoptic = 1 on the same chunk: that branch is above its cap as well
    assert re.search(r'sg_eval_class_tally\(\s*L\.ptr\(pred\), pk, L\.ptr\(sem\), sk, npts, int\(self\.ignore_label\), 1,',
                     _src(PKG, 'evaluation', 'panoptic_eval.py'))
    assert total > G.TALLY_CAP


def test_intersection_and_box_sizes_are_above_one_trip():
    cap = _launch_cap(_csrc('eval_ops.hip'), 'eval_intersections_kernel', 'total_points')
    assert cap == G.INTER_CAP == 8192 * 256
    # one run of 60 000, 20 000 single points, the other masks ~60 000 each (the GPU test asserts the exact total)
    assert G.INTER_MASK_POINTS + G.INTER_ISOLATED + (G.INTER_MASKS - 2) * G.INTER_MASK_POINTS * 0.95 > cap
    s = _csrc('det_eval.hip')
    runs, labels = _launch_cap(s, 'box_runs_kernel', 'total_points'), _launch_cap(s, 'box_labels_kernel', 'n_points')
    assert runs == labels == G.BOX_CAP == 8192 * 256
    assert G.BOX_SCANS * G.BOX_SCAN_POINTS > labels                           # points of one call
    assert (G.BOX_SCANS - 1) * G.BOX_SCAN_POINTS >= labels                    # the last scan starts in the second trip
    assert G.BOX_SCANS * G.BOX_MASKS * 3 * 25000 * 0.9 > runs                 # mask points (exact total: GPU test)
    # where the older test stops
    old = _src(HERE, 'test_box_eval_gpu.py')
    assert max(int(a) * int(b) for a, b in re.findall(r'\(np\.float\d+, \w+, \w+, (\d+), (\d+)\)', old)) == 300000 < labels


def test_train_data_sizes_are_above_the_block_cap():
    s = _csrc('train_data.hip')
    m = re.search(r'blocks_for\(int64_t n\)\s*\{\s*return sg::grid_for\(n, kBlock, (\d+)\);', s)
    assert m, 'blocks_for not found'
    cap = _const(s, 'kBlock') * int(m.group(1))
    assert cap == G.TRAIN_CAP == 262144
    # elastic, crop count and compaction see the whole scan; the S3DIS gather its quarter
    assert G.TRAIN_SCANNET_N > cap and int(G.TRAIN_S3DIS_N * 0.25) > cap
    assert cap < G.ELASTIC_N < 2 * cap and G.ELASTIC_N % 64                   # second trip, a partial last wave
    # quads of the x4 split and of the KITTI decode: blocks_for((n + 3) / 4)
    assert len(re.findall(r'blocks_for\(\(n \+ 3\) / 4\)', s)) == 3
    assert all((n + 3) // 4 > cap for n in G.X4_SIZES) and {n % 4 for n in G.X4_SIZES} == {0, 3}
    assert G.KITTI_CAP == 4 * cap and G.KITTI_CAP in G.KITTI_SIZES
    assert any(n > G.KITTI_CAP and n % 4 == 3 for n in G.KITTI_SIZES)
    assert G.UNALIGNED_N % 4 == 3 and G.UNALIGNED_N > 4 * 64
    # where the older tests are: 600 000 points above the cap (augment, id set, remap, offsets), the x4 split at
    # 1 000 003 points = 250 001 quads and the decode at 120 000 words below it
    old = _src(HERE, 'test_test_data_gpu.py')
    assert re.search(r'blobs\(600000, ', old) and 600000 > cap
    assert re.search(r'blobs\(1000003, ', old) and (1000003 + 3) // 4 <= cap
    m = re.search(r'def kitti_words\(n=(\d+),', _src(HERE, 'test_test_data.py'))
    assert m and (int(m.group(1)) + 3) // 4 <= cap
    m = re.search(r'def _scannet\(n=(\d+),', _src(HERE, 'test_train_data_gpu.py'))
    assert m and int(m.group(1)) == 150000 <= cap


def test_id_cap_is_half_the_table():
    s = _csrc('train_data.hip')
    m = re.search(r'constexpr\s+int\s+kIdTable\s*=\s*1\s*<<\s*(\d+)\s*;', s)
    assert m, 'kIdTable not found'
    table = 1 << int(m.group(1))
    assert re.search(r'cap <= kIdTable / 2', s)
    m = re.search(r'^_ID_CAP\s*=\s*(\d+)\s*$', _src(PKG, 'data', '_train_device.py'), re.M)
    assert m and int(m.group(1)) == table // 2 == G.ID_CAP
    assert G.ID_LABELS > G.ID_CAP + 1
