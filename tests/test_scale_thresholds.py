"""Keeps the sizes of tests/test_scale_thresholds_gpu.py honest: the thresholds are derived here from the constants
in the sources (one regular expression each), and every size the GPU tests use must sit on the side of its
threshold it was chosen for.  When a constant is retuned this test names the sizes to move, instead of the GPU tests
quietly no longer reaching the path."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_scale_thresholds_gpu as G  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'softgroup_amd', 'csrc')


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(src, name):
    m = re.search(r'constexpr\s+int\s+' + name + r'\s*=\s*(\d+)\s*;', src)
    assert m, f'constexpr int {name} not found'
    return int(m.group(1))


def _scan_limit():
    s = _src('scan.h')
    block, items, raw = (_const(s, k) for k in ('kScanBlock', 'kScanItems', 'kScanRawBlocks'))
    assert re.search(r'constexpr\s+int\s+kScanTile\s*=\s*kScanBlock\s*\*\s*kScanItems\s*;', s)
    assert re.search(r'if\s*\(\s*num_blocks\s*<=\s*kScanRawBlocks\s*\)', s)      # two launches up to here
    return block, block * items, raw * block * items


def _sort_limits():
    """([n above which keys per thread double ...], n above which the sort leaves its local-scan form, chunk)"""
    s = _src('radix_sort.h')
    block, items = _const(s, 'kRsBlock'), _const(s, 'kRsItems')
    m = re.search(r'while\s*\(\s*items\s*<\s*(\d+)\s*&&[^\n]*>\s*(\d+)\s*\)\s*\n\s*items\s*\*=\s*2\s*;', s)
    assert m, 'the loop that doubles `items` not found'
    cap, max_blocks = int(m.group(1)), int(m.group(2))
    m = re.search(r'local_scan\s*=\s*nblk\s*<=\s*(\d+)\s*&&\s*n_pass\s*<=\s*(\d+)\s*;', s)
    assert m, 'the local_scan condition not found'
    assert int(m.group(1)) == max_blocks and int(m.group(2)) >= 4      # (K = 27 sorts take 4 passes)
    steps, it = [], items
    while it < cap:
        steps.append(max_blocks * it * block)       # above this many pairs: 2 * it keys per thread
        it *= 2
    return steps, max_blocks * cap * block, cap


def test_scan_sizes_sit_on_both_sides_of_the_three_launch_form():
    block, tile, limit = _scan_limit()
    assert tile == G.SCAN_TILE and limit == 4194304, (tile, limit)
    sizes = G.SCAN_SIZES
    assert limit in sizes and limit - 1 in sizes and limit + 1 in sizes
    assert {0, 1, tile - 1, tile, tile + 1} <= set(sizes)
    # the chunk loop of scan_block_sums_kernel (kScanBlock block sums per chunk): ends on a full chunk, on a chunk
    # of one, and somewhere in between
    blocks = [(n + tile - 1) // tile for n in sizes if n > limit]
    assert any(b % block == 0 for b in blocks) and any(b % block == 1 for b in blocks)
    assert any(b % block not in (0, 1) for b in blocks)


def test_plan_sizes_cover_every_tile_size_of_the_sort():
    steps, local_limit, cap = _sort_limits()
    assert len(steps) == 3 and cap == 64, (steps, cap)
    rows27, rows8 = G.PLAN_SIZES[27], G.PLAN_SIZES[8]
    assert steps[0] in rows27 and steps[0] + 1 in rows27                    # the last 8-key size and the first 16-key
    assert any(steps[1] < r <= steps[2] for r in rows27)                    # 32 keys per thread
    assert any(steps[2] < r <= local_limit for r in rows27 + rows8)         # 64 keys per thread, 128 KB tile
    assert local_limit in rows8 and local_limit + 1 in rows8                # local scan: last size, first without
    assert steps[0] < G.OCTREE_N <= steps[1]                                # the octree's sort: 16 keys per thread


def test_pyramid_and_bfs_sizes_cross_their_gates():
    _, _, limit = _scan_limit()
    # 599 187 = the first M0 whose 7-level position scan is a three-launch scan (asserted on the scene in the test)
    assert G.PYRAMID_LEVELS * 599186 <= limit < G.PYRAMID_LEVELS * 599187
    s = _src('bfs.hip')
    vis = _const(s, 'kVisWords') * 32
    assert re.search(r'n\s*<=\s*kVisWords\s*\*\s*32', s)
    gates = re.findall(r'big_on\s*&&\s*n\s*<\s*\(1\s*<<\s*(\d+)\)', s)
    assert len(gates) == 2 and len(set(gates)) == 1, gates       # has_big and the per-cluster kernel's bound
    big = 1 << int(gates[0])
    big_min = _const(s, 'kOwnCap')
    assert re.search(r'constexpr\s+int\s+kBigMin\s*=\s*kOwnCap\s*;', s)
    assert vis < G.BFS_N_NOVIS < big <= G.BFS_N_PER_CLUSTER
    assert G.BFS_SHEET**2 > big_min and G.BFS_SLAB**2 > big_min and G.BFS_CLIQUE <= big_min
    # (below the visited filter's limit: the 62 500-point scene of tests/test_ops_gpu.py)
    assert 40000 + 22500 <= vis
