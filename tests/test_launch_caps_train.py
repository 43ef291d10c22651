"""Keeps the sizes of tests/test_launch_caps_train_gpu.py and of _sizes_above() in tests/test_fused_optim_gpu.py
honest: the launch caps of csrc/losses.hip, csrc/optim.hip, the mask-IoU part of csrc/seg_ops.hip and
csrc/instances.hip are derived here from the sources (one regular expression each), and every size the GPU tests
use must sit on the side of its cap it was chosen for.  When a grid or a block is retuned this test names the sizes
to move, instead of the GPU tests quietly making one trip through every loop again."""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import torch  # noqa: E402

_GPU_UP_BEFORE = torch.cuda.is_initialized()
import test_launch_caps_train_gpu as G  # noqa: E402

_GPU_UP_AFTER = torch.cuda.is_initialized()
import test_fused_optim_gpu as GO  # noqa: E402

_GPU_UP_AFTER_OPTIM = torch.cuda.is_initialized()

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


def _value(expr, names):
    """a block or grid argument such as `kLossBlock / kWave` or `4 * kLossMaxBlocks`"""
    assert re.fullmatch(r'[\w\s*/]+', expr), expr
    return int(eval(re.sub(r'/', '//', expr), {'__builtins__': {}}, dict(names)))


def _loss_names():
    s = _csrc('losses.hip')
    return dict(kLossBlock=_const(s, 'kLossBlock'), kLossMaxBlocks=_const(s, 'kLossMaxBlocks'),
                kWave=_const(_csrc('common.h'), 'kWave'))


def _cap(src, pattern, names):
    """items of one trip = block * max_blocks of the one `grid_for(<items>, block, max_blocks)` that `pattern`
    (two groups: block, max_blocks) finds"""
    found = re.findall(pattern, src)
    assert len(found) == 1, (pattern, found)
    return _value(found[0][0], names) * _value(found[0][1], names)


def test_importing_the_gpu_modules_does_not_touch_the_gpu():
    assert _GPU_UP_BEFORE or not (_GPU_UP_AFTER or _GPU_UP_AFTER_OPTIM)
    assert G.pytestmark.name == 'gpu' and GO.pytestmark.name == 'gpu'


def test_grid_for_caps_the_grid():
    assert re.search(r'inline int grid_for\(int64_t work_items, int block, int max_blocks = [^)]*\) \{\s*'
                     r'int64_t g = \(work_items \+ block - 1\) / block;\s*if \(g < 1\) g = 1;\s*'
                     r'if \(g > max_blocks\) g = max_blocks;', _csrc('common.h'))


# ----------------------------------------------------------------------------------------------------------------
def test_point_wise_sizes_sit_on_both_sides_of_the_grid_caps():
    s, names = _csrc('losses.hip'), _loss_names()
    m = re.search(r'static int pointwise_threads\(int c\) \{ return c <= (\d+) \? (\d+) : (\d+); \}', s)
    assert m, 'pointwise_threads not found'
    c_small, t_small, t_wide = (int(x) for x in m.groups())
    assert (c_small, t_small, t_wide) == (32, G._pw_tile(32), G._pw_tile(33))
    assert re.search(r'const int T = pointwise_threads\(c\);\s*const int grid = grid_for\(n, T, kLossMaxBlocks\);', s)
    m = re.search(r'pointwise_bwd_kernel<<<grid_for\(n, T, (\d+) \* kLossMaxBlocks\), T,', s)
    assert m, 'the launch of pointwise_bwd_kernel not found'
    fwd = {False: t_small * names['kLossMaxBlocks'], True: t_wide * names['kLossMaxBlocks']}      # keyed by c > 32
    bwd = {k: v * int(m.group(1)) for k, v in fwd.items()}
    assert (fwd[False], fwd[True], bwd[False], bwd[True]) == (G.PW_FWD_CAP, G.PW_FWD_CAP_WIDE, G.PW_BWD_CAP,
                                                              G.PW_BWD_CAP_WIDE)
    cases = G.PW_CASES
    assert cases[0][0] == fwd[False] and cases[1][0] == fwd[False] + 1 and cases[0][1] <= c_small >= cases[1][1]
    assert any(n > 2 * fwd[c > c_small] and n % G._pw_tile(c) and w for n, c, w in cases)        # third trip, partial tile
    assert any(fwd[True] < n and c > c_small for n, c, w in cases)                               # the T = 128 form
    assert any(n > bwd[True] and c > c_small and n % t_wide for n, c, w in cases)                # backward, both forms
    assert any(n > bwd[False] and c <= c_small and n % t_small for n, c, w in cases)
    assert {w for n, c, w in cases} == {False, True} and all(1 <= c <= _const(s, 'kLossMaxC') for n, c, w in cases)
    # where the older test stops
    old = _src(HERE, 'test_fused_losses_gpu.py')
    m = re.search(r'def test_point_wise_loss_shapes\(c\):\s*for n in \(([\d, ]+)\):', old)
    assert m and max(int(x) for x in m.group(1).split(',')) == 5000 < fwd[True]


def test_assignment_and_instance_loss_sizes_sit_on_both_sides_of_the_grid_caps():
    s, names = _csrc('losses.hip'), _loss_names()
    rows = _cap(s, r'const int rows_grid = grid_for\(n_proposal, ([\w /]+), (\w+)\);', names)
    cols = _cap(s, r'assign_cols_kernel<<<grid_for\(n_gt, ([\w /]+), (\w+)\), kLossBlock,', names)
    labels = _cap(s, r'assign_labels_kernel<<<grid_for\(n_proposal, (\w+), (\w+)\), kLossBlock,', names)
    p_fwd = _cap(s, r'const int grid = grid_for\(n_proposal, ([\w /]+), (\w+)\);\s*proposal_fwd_kernel<<<grid, kLossBlock,',
                 names)
    p_bwd = _cap(s, r'proposal_bwd_kernel<<<grid_for\(n_proposal, ([\w /]+), (\w+)\), kLossBlock,', names)
    m_fwd = _cap(s, r'const int grid = grid_for\(m, (\w+), (\w+)\);\s*mask_fwd_kernel<<<grid, kLossBlock,', names)
    m_bwd = _cap(s, r'mask_bwd_kernel<<<grid_for\(m \* k1, (\w+), ([\w *]+)\), kLossBlock,', names)
    assert rows == p_fwd == p_bwd == G.ROWS_CAP == 4096 and cols == G.COLS_CAP == 4096
    assert labels == m_fwd == G.LABELS_CAP == 262144 and m_bwd == G.MASK_BWD_CAP == 8 * 262144
    # one wave per proposal / GT column
    assert len(re.findall(r'p = blockIdx\.x \* \(kLossBlock / kWave\) \+ \(threadIdx\.x >> 6\); p < n_prop;', s)) == 3
    assert len(re.findall(r'g = blockIdx\.x \* \(kLossBlock / kWave\) \+ \(threadIdx\.x >> 6\); g < n_gt;', s)) == 1
    a = G.ASSIGN_CASES
    assert a[0][0] == rows and a[1][0] == rows + 1 and a[2][0] > 2 * rows and a[2][0] % 64
    assert a[3][1] > cols and a[3][0] < rows and a[4][0] > labels
    assert all(n_gt <= cols for n_prop, n_gt in a[:3] + a[4:])
    i = G.INST_CASES
    assert i[0][0] > rows and i[0][2] > m_fwd and i[0][2] % 256 and i[0][2] * i[0][1] > 2 * m_bwd       # third trip of mask_bwd
    assert i[1][0] > rows and i[1][1] == 2 and m_bwd < i[1][2] * i[1][1] < 2 * m_bwd                      # its second at k1 = 2
    assert i[2][0] == rows and i[2][2] == m_fwd and i[2][2] * i[2][1] > m_bwd
    assert all(2 <= k1 <= _const(s, 'kLossMaxC') for n_prop, k1, m in i)
    # where the older tests stop: 300 proposals, 130 GT columns, 20 000 mask points of 19 columns
    old = _src(HERE, 'test_fused_losses_gpu.py')
    props = [max(int(x) for x in lst.split(',')) for lst in re.findall(r"parametrize\('n_prop', \[([\d, ]+)\]\)", old)]
    assert props == [300, 300] and 300 < rows
    m = re.search(r'for n_gt in \(([\d, ]+)\):', old)
    assert m and max(int(x) for x in m.group(1).split(',')) == 130 < cols
    m = re.search(r'for m in \(([\d, ]+)\):', old)
    k1 = re.search(r"parametrize\('k1', \[([\d, ]+)\]\)", old)
    assert m and k1
    m_old, k1_old = max(int(x) for x in m.group(1).split(',')), max(int(x) for x in k1.group(1).split(','))
    assert m_old == 20000 < m_fwd and m_old * k1_old == 380000 < m_bwd


# ----------------------------------------------------------------------------------------------------------------
def test_optimizer_sizes_are_above_the_chunk_walk_caps():
    s = _csrc('optim.hip')
    step_cap, norm_cap = _const(s, 'kOptMaxBlocks'), _const(s, 'kOptNormBlocks')
    assert (step_cap, norm_cap) == (GO.STEP_CAP, GO.NORM_CAP) == (2048, 1024)
    assert re.search(r'constexpr int kOptChunk = kOptBlock \* kOptQuads \* 4;', s)
    chunk = _const(s, 'kOptBlock') * _const(s, 'kOptQuads') * 4
    assert chunk == GO.O.chunk_elems() == 8192
    assert re.search(r'const int grid = static_cast<int>\(n_chunks < kOptNormBlocks \? n_chunks : kOptNormBlocks\);', s)
    assert re.search(r'step_grid\(int64_t n_chunks\) \{ return static_cast<int>\(n_chunks < kOptMaxBlocks \? n_chunks : '
                     r'kOptMaxBlocks\); \}', s)
    assert len(re.findall(r'<<<step_grid\(n_chunks\), kOptBlock,', s)) == 4       # adam, sgd with and without m, scale
    assert len(re.findall(r'for \(int64_t c = blockIdx\.x; c < n_chunks; c \+= gridDim\.x\)', s)) == 4

    def chunks_of(sizes):                                   # sg_optim_plan: tensor of every chunk, in order
        return np.repeat(np.arange(len(sizes)), [-(-n // chunk) for n in sizes])

    above = chunks_of(GO._sizes_above())
    assert len(above) == len(GO.O.plan_chunks(GO._sizes_above()))
    assert len(above) > step_cap and len(above) > 2 * norm_cap and sum(GO._sizes_above()) < 300000
    big = np.flatnonzero(above == GO._sizes_above().index(4 * chunk + 1))
    assert len(big) == 5 and big[0] < step_cap <= big[-1]                       # `arrive` counts in two trips
    assert all(GO._sizes_above()[i] == 5 for i in GO.VIEWS)
    # where the older inputs stop: about 720 chunks
    assert 700 < len(chunks_of(GO._sizes())) < min(norm_cap, step_cap)
    # chunk_done: one barrier in front of both branches
    m = re.search(r'void chunk_done\(.*?\n\}', s, re.S)
    assert m and re.search(r'kOptChunk;\s*__syncthreads\(\);\s*if \(n_of_tensor <= 1\)', m.group(0))


# ----------------------------------------------------------------------------------------------------------------
def test_mask_iou_sizes_are_above_the_proposal_and_bin_caps():
    s = _csrc('seg_ops.hip')
    grids = re.findall(r'mask_(?:iou_kernel<(?:false|true)>|label_kernel)<<<min\(nProposal, (\d+)\), 256,', s)
    assert grids == ['8192'] * 3
    bins = _const(s, 'kIouBins')
    assert int(grids[0]) == G.IOU_PROP_CAP and bins == G.IOU_BINS
    assert re.search(r'for \(int g0 = 0; g0 < nInstance; g0 \+= kIouBins\)', s)
    assert G.IOU_MANY_PROPOSALS['nP'] > G.IOU_PROP_CAP and G.IOU_MANY_PROPOSALS['nI'] < bins
    assert G.IOU_MANY_INSTANCES['nI'] > bins and G.IOU_MANY_INSTANCES['nI'] > 256 * 32 > G.IOU_MANY_INSTANCES['nP']
    # where the older test stops
    m = re.search(r'def test_mask_iou_and_label\(\):\s*rng = [^\n]*\n\s*N, nI, nP = (\d+), (\d+), (\d+)',
                  _src(HERE, 'test_ops_gpu.py'))
    assert m and int(m.group(2)) == 37 < bins and int(m.group(3)) == 90 < int(grids[0])


def test_instance_sizes_are_above_one_trip():
    s = _csrc('instances.hip')
    m = re.search(r'const int grid = grid_for\(\(S \+ 63\) / 64, (\d+), (\d+)\);\s*instance_npoint_kernel<<<grid, 256,', s)
    assert m, 'the launch of instance_npoint_kernel not found'
    waves = int(m.group(1)) * int(m.group(2))
    assert waves == G.NPOINT_WAVES and waves * 64 == G.NPOINT_ONE_CHUNK_CAP
    assert re.search(r'const int64_t n_waves = static_cast<int64_t>\(gridDim\.x\) \* 4;\s*'
                     r'const int64_t per = \(\(\(S \+ n_waves - 1\) / n_waves\) \+ 63\) & ~63LL;', s)
    bitmap = re.search(r'const int grid = grid_for\(S, (\d+), (\d+)\);\s*instance_bitmap_kernel<<<grid, 256,', s)
    emit = re.search(r'instance_runs_emit_kernel<<<grid_for\(tw, (\d+), (\d+)\), 256,', s)
    text = re.search(r'rle_text_kernel<<<grid_for\(n, (\d+), (\d+)\), 256,', s)
    assert bitmap and emit and text
    assert {int(x.group(1)) * int(x.group(2)) for x in (bitmap, emit, text)} == {G.RUNS_CAP}
    # sg_instance_npoint: every wave walks at least four chunks, the trailing waves start behind the last pair
    sizes, dead = G._npoint_layout()
    S = int(sizes.sum())
    per = G.npoint_wave_range(S)
    assert G.NPOINT_MIN_PAIRS == waves * 192 and G.npoint_wave_range(G.NPOINT_MIN_PAIRS) == 192
    assert S > G.NPOINT_MIN_PAIRS and per >= 256 and S % 64 == 7 and (waves - 1) * per >= S
    assert sizes[0] == G.NPOINT_GIANT >= 149000 and sizes[dead] == G.NPOINT_BLOCKS['dead']
    assert {nc > 8 for nc, stride in G.NPOINT_CLASSES} == {False, True}          # the `i0 += 8` class rounds
    assert all(nc <= stride and nc <= 64 for nc, stride in G.NPOINT_CLASSES)
    # sg_instance_runs: pairs, bitmap words and (in the GPU test, from its reference) runs above one trip
    words = (G.RUNS_POINTS + 31) // 32
    assert G.RUNS_PROPOSALS * G.RUNS_PER_PROPOSAL > G.RUNS_CAP and (G.RUNS_PROPOSALS - 2) * words > G.RUNS_CAP
    assert G.RUNS_PER_PROPOSAL * 32 <= G.RUNS_POINTS                             # sparse rows: nearly every point a run
    # where the older test stops: 23 proposals of at most 3 ranges of 400 points and 30 single ones, one full row
    m = re.search(r'def test_instance_npoint_and_runs_vs_dense_masks\(\):.*?N, nP, nc, stride = (\d+), (\d+), (\d+), (\d+)',
                  _src(HERE, 'test_ops_gpu.py'), re.S)
    assert m
    n, n_prop, nc, _ = (int(x) for x in m.groups())
    assert n_prop * (3 * 400 + 30) + n < G.NPOINT_ONE_CHUNK_CAP and nc == 5 and n == 5000
