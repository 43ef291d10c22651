"""Every launch form of the training convolution (csrc/spconv_train.hip) against the float64 reference of
tests/conv_ref.py on gather tables from the CPU oracle: the bf16 forward / input-gradient kernel
(sg_spconv_gather_conv_bf16), the weight gradient (sg_spconv_wgrad) and the bf16 weight packing.

Nothing on the reference side comes from the library.  Both launch decisions are pure functions of the shape, so
every form is named with a fixed row count, and every case first ASKS the library
(sg_spconv_conv_bf16_launch_info / sg_spconv_wgrad_launch_info: the launch path's own decision) and asserts the
form it is named for.  tests/test_train_conv_ref.py keeps the case lists complete against the source and checks
the conditions the tables were built for, without a GPU.

Common to all cases: operand magnitudes in [0.25, 4] with random signs (within a factor of 4 of unit scale: one
missing or doubled product moves an element by at least 1/16, some thousand times either bar; the 1e-3 .. 1e3 row
scales of the inference test would hide a lost small row inside a long sum); outputs NaN-filled with 64 poisoned spare rows behind them; the
workspace is the test's own, NaN-filled, with a guard pattern behind its queried size; every call runs twice and
the two results are bit-identical.

Forward and input gradient (bf16 out), per element, against float64 on the bf16-rounded operands.  Rounding is
monotone, so an fp32 sum within E of the reference must land inside the bracket
    round_bf16(ref - E) <= got <= round_bf16(ref + E)
  * ceiling, any summation order:  E = (n + ksplit) 2^-24 S_abs
  * working bar:                   E_w = max(1e-5, 4 e32) max|ref row|, e32 the row error of a float32 torch
    evaluation of the same reference (the two numbers of tests/test_conv_ref_gpu.py).
Weight gradient (fp32 out), per offset slice k, against conv_ref.wgrad on the operands as given:
  * ceiling:      |got - ref| <= (n[k] + 8) 2^-24 S_abs
  * working bar:  max|got - ref| / max|ref[k]| <= max(1e-5, 4 e32_k), e32_k from a float32 torch gather + matmul
  * a slice with no pair is exactly zero.

Measured on an MI355X, printed by every case: `flips` = share of elements with got != round_bf16(ref), `mid` = the
largest distance of such an element's reference from its rounding midpoint over the row maximum, `err` = largest
error of an offset slice over that slice's largest |ref|.

MEASURED (plan and table runs gave identical lines throughout; form = (col_units, blocks_per_unit, vec, ksplit,
k_per_split) for the bf16 kernel, (vi, vo, nst, zs, rows, chunks, csplit, rs) for the weight gradient)

  forward / input gradient      K Cin->Cout  rows        form                e32       flips     mid
  subm_1024_tiles   27  32->32  32737  no ws (1, 1, 1, 1, 27)    2.62e-07  2.86e-06  3.63e-08
  subm_1023_tiles   27  32->32  32705  ws    (1, 1, 1, 2, 14)    2.83e-07  5.73e-06  3.43e-08
  subm_bpu4_last3   27  16->224 16353  ws    (2, 4, 1, 1, 27)    1.96e-07  5.46e-07  3.27e-08
  subm_bpu3_split4  27  48->96   8161  ws    (1, 3, 1, 4, 7)     2.39e-07  1.15e-05  3.87e-08
  subm_bpu4_split7  27  64->128  4065  ws    (1, 4, 1, 7, 4)     1.61e-07  0.00e+00  0.00e+00
  subm_elem_3_2     27  40->160  6000  ws    (2, 3, 0, 3, 9)     2.66e-07  4.17e-06  8.14e-08
  subm_elem_3x3     27  20->288  5000  ws    (3, 3, 0, 3, 9)     2.18e-07  0.00e+00  0.00e+00
  subm_odd_cin      27   7->40   2000  ws    (1, 2, 0, 14, 2)    0.00e+00  0.00e+00  0.00e+00
  subm_27_ranges    27  32->32    141  ws    (1, 1, 1, 27, 1)    1.19e-07  0.00e+00  0.00e+00
  subm_27_ranges    27  32->32    141  no ws (1, 1, 1, 1, 27)    1.19e-07  0.00e+00  0.00e+00
  subm_bpu1_elem    27   6->32    141  ws    (1, 1, 0, 27, 1)    5.47e-08  0.00e+00  0.00e+00
  subm_bpu4_elem    27  24->128   141  ws    (1, 4, 0, 27, 1)    1.37e-07  0.00e+00  0.00e+00
  down_8_ranges      8  64->96    141  ws    (1, 3, 1, 8, 1)     1.33e-07  7.39e-05  2.65e-08
  down_split_332     8  96->64  12000  ws    (1, 2, 1, 3, 3)     2.10e-07  2.47e-05  8.47e-08
  up_no_tap_rows     8 128->96   3001  ws    (1, 3, 1, 8, 1)     2.50e-07  0.00e+00  0.00e+00
  one_1_item         1  16->32    141  ws    (1, 1, 1, 1, 1)     0.00e+00  0.00e+00  0.00e+00
  one_2_items        1  32->6     141  ws    (1, 1, 1, 1, 1)     0.00e+00  0.00e+00  0.00e+00
  one_20_items       1 320->160   141  ws    (2, 3, 1, 1, 1)     4.62e-07  0.00e+00  0.00e+00
  module_subm_32_64 dgrad                     (1, 1, 1, 9, 3)     2.52e-07  3.12e-05  2.34e-08
  module_subm_20_36 dgrad                     (1, 1, 0, 9, 3)     2.43e-07  0.00e+00  0.00e+00
  module_down_32_64 dgrad                     (1, 1, 1, 8, 1)     1.31e-07  0.00e+00  0.00e+00
  module_down_20_36 dgrad                     (1, 1, 0, 8, 1)     6.07e-08  0.00e+00  0.00e+00
  module_up_32_64 dgrad                       (1, 1, 1, 8, 1)     1.32e-07  0.00e+00  0.00e+00
  module_up_20_36 dgrad                       (1, 1, 0, 8, 1)     1.06e-07  0.00e+00  0.00e+00

No element left either bracket.  At most 7e-5 of the elements differ from round_bf16(ref) at all, and each of those
has its reference within 9e-8 of the row maximum of a rounding midpoint -- below e32: the fp32 sum fell on the
other side of the midpoint, nothing else.

  weight gradient   K Cin->Cout  rows  in/g       form                             err       e32
  inst_32_32      27  32->32    141  fp32/fp32  (1, 1, 1, 1, 128, 2, 1, 4)       1.44e-07  3.51e-07
  inst_32_32      27  32->32    141  fp32/bf16  (1, 1, 1, 1, 128, 2, 1, 4)       1.73e-07  3.52e-07
  inst_32_32      27  32->32    141  bf16/fp32  (1, 1, 1, 1, 128, 2, 1, 4)       1.45e-07  3.51e-07
  inst_32_32      27  32->32    141  bf16/bf16  (1, 1, 1, 1, 128, 2, 1, 4)       6.76e-08  1.01e-07
  inst_6_32       27   6->32    141  fp32/fp32  (1, 1, 1, 1, 128, 2, 1, 4)       1.36e-07  1.22e-07
  inst_6_32       27   6->32    141  fp32/bf16  (1, 1, 1, 1, 128, 2, 1, 4)       1.40e-07  1.29e-07
  inst_6_32       27   6->32    141  bf16/fp32  (1, 1, 1, 1, 128, 2, 1, 4)       1.38e-07  1.08e-07
  inst_6_32       27   6->32    141  bf16/bf16  (1, 1, 1, 1, 128, 2, 1, 4)       3.47e-08  6.94e-08
  inst_32_48      27  32->48    141  fp32/fp32  (1, 1, 2, 1, 128, 2, 1, 2)       2.28e-07  3.67e-07
  inst_32_48      27  32->48    141  fp32/bf16  (1, 1, 2, 1, 128, 2, 1, 2)       2.71e-07  6.98e-07
  inst_32_48      27  32->48    141  bf16/fp32  (1, 1, 2, 1, 128, 2, 1, 2)       1.99e-07  4.41e-07
  inst_32_48      27  32->48    141  bf16/bf16  (1, 1, 2, 1, 128, 2, 1, 2)       7.18e-08  1.44e-07
  inst_7_33       27   7->33    141  fp32/fp32  (1, 1, 2, 1, 128, 2, 1, 2)       1.67e-07  1.47e-07
  inst_7_33       27   7->33    141  fp32/bf16  (1, 1, 2, 1, 128, 2, 1, 2)       1.60e-07  1.32e-07
  inst_7_33       27   7->33    141  bf16/fp32  (1, 1, 2, 1, 128, 2, 1, 2)       1.77e-07  1.34e-07
  inst_7_33       27   7->33    141  bf16/bf16  (1, 1, 2, 1, 128, 2, 1, 2)       4.15e-08  4.15e-08
  inst_64_32      27  64->32    141  fp32/fp32  (2, 1, 1, 1, 128, 2, 1, 4)       1.30e-07  5.84e-07
  inst_64_32      27  64->32    141  fp32/bf16  (2, 1, 1, 1, 128, 2, 1, 4)       1.82e-07  3.42e-07
  inst_64_32      27  64->32    141  bf16/fp32  (2, 1, 1, 1, 128, 2, 1, 4)       1.85e-07  4.02e-07
  inst_64_32      27  64->32    141  bf16/bf16  (2, 1, 1, 1, 128, 2, 1, 4)       6.88e-08  1.03e-07
  inst_32_64      27  32->64    141  fp32/fp32  (1, 2, 1, 1, 128, 2, 1, 4)       1.25e-07  3.84e-07
  inst_32_64      27  32->64    141  fp32/bf16  (1, 2, 1, 1, 128, 2, 1, 4)       1.99e-07  3.76e-07
  inst_32_64      27  32->64    141  bf16/fp32  (1, 2, 1, 1, 128, 2, 1, 4)       1.34e-07  3.14e-07
  inst_32_64      27  32->64    141  bf16/bf16  (1, 2, 1, 1, 128, 2, 1, 4)       8.77e-08  1.17e-07
  inst_96_96      27  96->96    141  fp32/fp32  (2, 2, 4, 1, 128, 2, 1, 1)       3.73e-07  3.99e-07
  inst_96_96      27  96->96    141  fp32/bf16  (2, 2, 4, 1, 128, 2, 1, 1)       4.35e-07  3.79e-07
  inst_96_96      27  96->96    141  bf16/fp32  (2, 2, 4, 1, 128, 2, 1, 1)       4.05e-07  4.84e-07
  inst_96_96      27  96->96    141  bf16/bf16  (2, 2, 4, 1, 128, 2, 1, 1)       8.26e-08  1.10e-07
  inst_40_72      27  40->72    141  fp32/fp32  (1, 2, 4, 1, 128, 2, 1, 1)       2.89e-07  3.94e-07
  inst_40_72      27  40->72    141  fp32/bf16  (1, 2, 4, 1, 128, 2, 1, 1)       3.80e-07  3.70e-07
  inst_40_72      27  40->72    141  bf16/fp32  (1, 2, 4, 1, 128, 2, 1, 1)       3.34e-07  3.34e-07
  inst_40_72      27  40->72    141  bf16/bf16  (1, 2, 4, 1, 128, 2, 1, 1)       1.01e-07  1.01e-07
  inst_192_96     27 192->96    141  fp32/fp32  (2, 2, 6, 2, 128, 2, 1, 1)       3.70e-07  4.32e-07
  inst_192_96     27 192->96    141  fp32/bf16  (2, 2, 6, 2, 128, 2, 1, 1)       3.96e-07  4.27e-07
  inst_192_96     27 192->96    141  bf16/fp32  (2, 2, 6, 2, 128, 2, 1, 1)       3.46e-07  3.96e-07
  inst_192_96     27 192->96    141  bf16/bf16  (2, 2, 6, 2, 128, 2, 1, 1)       1.00e-07  1.00e-07
  inst_160_224    27 160->224   141  fp32/fp32  (2, 2, 12, 3, 128, 2, 1, 1)      4.09e-07  4.31e-07
  inst_160_224    27 160->224   141  fp32/bf16  (2, 2, 12, 3, 128, 2, 1, 1)      4.06e-07  4.06e-07
  inst_160_224    27 160->224   141  bf16/fp32  (2, 2, 12, 3, 128, 2, 1, 1)      3.01e-07  3.43e-07
  inst_160_224    27 160->224   141  bf16/bf16  (2, 2, 12, 3, 128, 2, 1, 1)      9.39e-08  9.39e-08
  rows_1          27  32->32      1  fp32/fp32  (1, 1, 1, 1, 128, 1, 1, 4)       3.07e-08  3.07e-08
  rows_1          27  32->32      1  bf16/bf16  (1, 1, 1, 1, 128, 1, 1, 4)       0.00e+00  0.00e+00
  rows_129        27  32->32    129  fp32/fp32  (1, 1, 1, 1, 128, 2, 1, 4)       1.13e-07  3.08e-07
  rows_129        27  32->32    129  bf16/bf16  (1, 1, 1, 1, 128, 2, 1, 4)       6.32e-08  6.32e-08
  rows_4865       27  32->32   4865  fp32/fp32  (1, 1, 1, 1, 130, 38, 1, 4)      1.75e-07  1.94e-06
  rows_4865       27  32->32   4865  bf16/bf16  (1, 1, 1, 1, 130, 38, 1, 4)      1.54e-07  1.55e-06
  rows_9738       27  32->32   9738  fp32/fp32  (1, 1, 1, 1, 258, 38, 4, 4)      1.68e-07  4.74e-06
  rows_9738       27  32->32   9738  bf16/bf16  (1, 1, 1, 1, 258, 38, 4, 4)      1.59e-07  2.23e-06
  rows_9761_2x2   27  64->64   9761  fp32/fp32  (2, 2, 1, 1, 258, 38, 4, 4)      1.85e-07  2.85e-06
  rows_9761_2x2   27  64->64   9761  bf16/bf16  (2, 2, 1, 1, 258, 38, 4, 4)      1.62e-07  2.14e-06
  rows_78000      27  32->32  78000  fp32/fp32  (1, 1, 1, 1, 2048, 39, 4, 4)     3.07e-07  6.61e-06
  rows_78000      27  32->32  78000  bf16/bf16  (1, 1, 1, 1, 2048, 39, 4, 4)     1.54e-07  5.39e-06
  rows_26700_zs3  27 160->224 26700  fp32/fp32  (2, 2, 12, 3, 2048, 14, 4, 1)    5.97e-07  4.42e-06
  rows_26700_zs3  27 160->224 26700  bf16/bf16  (2, 2, 12, 3, 2048, 14, 4, 1)    3.02e-07  4.08e-06
  down_141         8  64->96    141  fp32/fp32  (2, 2, 2, 1, 128, 2, 1, 2)       2.33e-07  3.85e-07
  down_141         8  64->96    141  bf16/bf16  (2, 2, 2, 1, 128, 2, 1, 2)       6.91e-08  1.24e-07
  down_20000       8  64->96  20000  fp32/fp32  (2, 2, 2, 1, 158, 127, 1, 2)     2.16e-07  5.15e-06
  down_20000       8  64->96  20000  bf16/bf16  (2, 2, 2, 1, 158, 127, 1, 2)     1.64e-07  3.64e-06
  up_3001          8 128->96   3001  fp32/fp32  (2, 2, 4, 1, 128, 24, 1, 1)      1.73e-07  8.08e-07
  up_3001          8 128->96   3001  bf16/bf16  (2, 2, 4, 1, 128, 24, 1, 1)      1.07e-07  3.24e-07
  one_141_zs4      1 320->160   141  fp32/fp32  (2, 2, 15, 4, 128, 2, 1, 1)      4.49e-07  4.49e-07
  one_141_zs4      1 320->160   141  bf16/bf16  (2, 2, 15, 4, 128, 2, 1, 1)      1.09e-07  1.37e-07
  one_3000         1  64->32   3000  fp32/fp32  (2, 1, 1, 1, 128, 24, 1, 4)      1.14e-07  1.59e-06
  one_3000         1  64->32   3000  bf16/bf16  (2, 1, 1, 1, 128, 24, 1, 4)      7.96e-08  1.03e-06
  module_subm_32_64 wgrad                  (1, 2, 1, 1, 128, 24, 1, 4)      1.32e-07  1.02e-06
  module_subm_20_36 wgrad                  (1, 1, 2, 1, 128, 24, 1, 2)      1.08e-07  9.63e-07
  module_down_32_64 wgrad                  (1, 2, 1, 1, 128, 8, 1, 4)       6.35e-08  2.75e-07
  module_down_20_36 wgrad                  (1, 1, 2, 1, 128, 8, 1, 2)       8.72e-08  3.84e-07
  module_up_32_64 wgrad                    (1, 2, 1, 1, 128, 24, 1, 4)      8.68e-08  2.44e-07
  module_up_20_36 wgrad                    (1, 1, 2, 1, 128, 24, 1, 2)      9.56e-08  2.31e-07

Every form sits under the working bar, so the chunk-by-chunk float32 re-accumulation of the reference that
would explain a form between the bar and the ceiling was not needed.  The kernel's error stays at 1e-7 .. 6e-7
where the float32 torch matmul over the same pairs reaches 7e-6 at 78000 rows: chunk sums of at most 2048 rows,
added in chunk order.
"""
import functools
import os
import sys
import zlib
from collections import namedtuple

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref  # noqa: E402
import test_conv_ref_gpu as G  # noqa: E402  (table builders shared with the inference cases)
from unet_train_ref import exact_voxels  # noqa: E402

from softgroup_amd.spconv import core  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SPARE = 64                      # poisoned rows behind every output
GUARD = 4096                    # bytes of guard pattern behind every workspace
KVOL = G.KVOL
U32 = conv_ref.U32

# ---------------------------------------------------------------------------------------------------
# case lists (pure data: tests/test_train_conv_ref.py reads them on the CPU)
# ---------------------------------------------------------------------------------------------------
# want: what sg_spconv_conv_bf16_launch_info must report with the full workspace -- (col_units, blocks_per_unit,
# vec, ksplit, k_per_split); nows: the same without a workspace (only where the case runs that way too)
# flags: 'empty_range' a (tile, offset range) without any neighbour; 'residues' item counts of all residues mod
# kRing; 'no_tap' rows without a tap; density = share of the grid's cells that are occupied (subm only)
FCase = namedtuple('FCase', 'name kind cin cout rows want nows flags density')


def _fcases():
    out = []

    def add(name, kind, cin, cout, rows, want, nows=None, flags=(), density=0.3):
        out.append(FCase(name, kind, cin, cout, rows, want, nows, tuple(flags), density))

    add('subm_1024_tiles', 'subm', 32, 32, 32737, (1, 1, 1, 1, 27))                  # 1024 tiles, no split
    add('subm_1023_tiles', 'subm', 32, 32, 32705, (1, 1, 1, 2, 14), flags=['residues'])      # split 14 + 13
    add('subm_bpu4_last3', 'subm', 16, 224, 16353, (2, 4, 1, 1, 27))                 # last unit 3 blocks, one slice
    add('subm_bpu3_split4', 'subm', 48, 96, 8161, (1, 3, 1, 4, 7))                   # 7/7/7/6
    add('subm_bpu4_split7', 'subm', 64, 128, 4065, (1, 4, 1, 7, 4), flags=['residues'], density=0.03)       # 4 x 6 + 3
    add('subm_elem_3_2', 'subm', 40, 160, 6000, (2, 3, 0, 3, 9))                     # units of 3 + 2 blocks, 9/9/9
    add('subm_elem_3x3', 'subm', 20, 288, 5000, (3, 3, 0, 3, 9))                     # 3 units of 3
    add('subm_odd_cin', 'subm', 7, 40, 2000, (1, 2, 0, 14, 2), flags=['residues'], density=0.03)   # 8-column last block, 13 x 2 + 1
    add('subm_27_ranges', 'subm', 32, 32, 141, (1, 1, 1, 27, 1), nows=(1, 1, 1, 1, 27), flags=['empty_range'],
        density=0.08)
    add('subm_bpu1_elem', 'subm', 6, 32, 141, (1, 1, 0, 27, 1))                      # launch_bf16<1>, element loads
    add('subm_bpu4_elem', 'subm', 24, 128, 141, (1, 4, 0, 27, 1))                    # launch_bf16<4>, element loads
    add('down_8_ranges', 'down', 64, 96, 141, (1, 3, 1, 8, 1))
    add('down_split_332', 'down', 96, 64, 12000, (1, 2, 1, 3, 3))                    # 3/3/2
    add('up_no_tap_rows', 'up', 128, 96, 3001, (1, 3, 1, 8, 1), flags=['no_tap'])
    add('one_1_item', 'one', 16, 32, 141, (1, 1, 1, 1, 1))
    add('one_2_items', 'one', 32, 6, 141, (1, 1, 1, 1, 1))
    add('one_20_items', 'one', 320, 160, 141, (2, 3, 1, 1, 1))
    return out


FCASES = _fcases()

# want: (vi, vo, nst, zs, rows, chunks, csplit, rs) of sg_spconv_wgrad_launch_info
# types: (in is bf16, g is bf16) pairs to run
# flags: 'empty_pair' a (chunk, offset) with no pair; 'odd' a chunk with an odd pair count; 'single' a chunk with
# exactly one pair; 'empty_piece' a centre chunk whose last piece gets no row
WCase = namedtuple('WCase', 'name kind cin cout rows want types flags')
ALL_TYPES = ((0, 0), (0, 1), (1, 0), (1, 1))
TWO_TYPES = ((0, 0), (1, 1))


def _wcases():
    out = []

    def add(name, kind, cin, cout, rows, want, types=TWO_TYPES, flags=()):
        out.append(WCase(name, kind, cin, cout, rows, want, types, tuple(flags)))

    # instantiations and meetings: K = 27, 141 rows, all four operand type pairs
    for cin, cout, vi, vo, nst, zs, rs in ((32, 32, 1, 1, 1, 1, 4), (6, 32, 1, 1, 1, 1, 4), (32, 48, 1, 1, 2, 1, 2),
                                           (7, 33, 1, 1, 2, 1, 2), (64, 32, 2, 1, 1, 1, 4), (32, 64, 1, 2, 1, 1, 4),
                                           (96, 96, 2, 2, 4, 1, 1), (40, 72, 1, 2, 4, 1, 1), (192, 96, 2, 2, 6, 2, 1),
                                           (160, 224, 2, 2, 12, 3, 1)):
        add(f'inst_{cin}_{cout}', 'subm', cin, cout, 141, (vi, vo, nst, zs, 128, 2, 1, rs), ALL_TYPES)
    # row classes
    add('rows_1', 'subm', 32, 32, 1, (1, 1, 1, 1, 128, 1, 1, 4), flags=['single'])
    add('rows_129', 'subm', 32, 32, 129, (1, 1, 1, 1, 128, 2, 1, 4), flags=['single', 'odd', 'empty_pair'])
    add('rows_4865', 'subm', 32, 32, 4865, (1, 1, 1, 1, 130, 38, 1, 4))
    add('rows_9738', 'subm', 32, 32, 9738, (1, 1, 1, 1, 258, 38, 4, 4), flags=['empty_piece'])
    add('rows_9761_2x2', 'subm', 64, 64, 9761, (2, 2, 1, 1, 258, 38, 4, 4))
    add('rows_78000', 'subm', 32, 32, 78000, (1, 1, 1, 1, 2048, 39, 4, 4), flags=['empty_piece'])
    add('rows_26700_zs3', 'subm', 160, 224, 26700, (2, 2, 12, 3, 2048, 14, 4, 1))
    # other kernel volumes
    add('down_141', 'down', 64, 96, 141, (2, 2, 2, 1, 128, 2, 1, 2))
    add('down_20000', 'down', 64, 96, 20000, (2, 2, 2, 1, 158, 127, 1, 2))
    add('up_3001', 'up', 128, 96, 3001, (2, 2, 4, 1, 128, 24, 1, 1))
    add('one_141_zs4', 'one', 320, 160, 141, (2, 2, 15, 4, 128, 2, 1, 1))
    add('one_3000', 'one', 64, 32, 3000, (2, 1, 1, 1, 128, 24, 1, 4))
    return out


WCASES = _wcases()

# the modules under bf16 autocast: (kind, Cin, Cout); 20 -> 36 takes the element-load path both ways
MCASES = [(kind, cin, cout) for kind in ('subm', 'down', 'up') for cin, cout in ((32, 64), (20, 36))]
MROWS = 3001


# ---------------------------------------------------------------------------------------------------
# tables (CPU oracle) and operands
# ---------------------------------------------------------------------------------------------------
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


@functools.lru_cache(maxsize=4)
def tables(name, kind, rows, density=0.3):
    """oracle gather table with exactly `rows` output rows -> (table [rows, K] int32, input rows)"""
    rng = _rng(name)
    if kind == 'subm':
        if rows < 8:
            ext = [3, 3, 3]
        else:
            ext = G._extent(rows / density)
        idx = exact_voxels(rng, rows, ext, 1)
        return conv_ref.subm_table(idx, ext), rows
    if kind == 'up':                    # odd extents: the rows on the dropped last planes have no tap
        ext = G._extent(rows / 0.4)
        assert all(e % 2 == 1 for e in ext)
        idx = exact_voxels(rng, rows, ext, 1)
        _, up, m_parents = conv_ref.down_tables(idx, ext)
        return up, m_parents
    return G._tables(kind, rows, rng)


def form_f(info):
    return (info.col_units, info.blocks_per_unit, info.vec, info.ksplit, info.k_per_split)


def form_w(info):
    return (info.vi, info.vo, info.nst, info.zs, info.rows, info.chunks, info.csplit, info.rs)


def _vals(shape, gen):
    """magnitudes in [0.25, 4] (log-uniform), random signs"""
    mag = torch.exp2(torch.rand(shape, device=DEV, generator=gen) * 4 - 2)
    sign = torch.randint(0, 2, shape, device=DEV, generator=gen).float() * 2 - 1
    return mag * sign


def _gen(name):
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(name.encode()))


def _workspace(nbytes):
    """NaN-filled workspace of `nbytes` with a guard pattern behind it -> (buffer, check())"""
    nbytes = (int(nbytes) + 3) // 4 * 4
    buf = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=DEV)
    buf[:nbytes].view(torch.float32).fill_(float('nan'))
    buf[nbytes:] = 0xA5

    def check(used=None):
        assert bool((buf[nbytes:] == 0xA5).all()), 'guard behind the workspace overwritten'
        if used is not None:
            used = (int(used) + 3) // 4 * 4
            assert bool(torch.isnan(buf[used:nbytes].view(torch.float32)).all()), 'workspace written past what the query reports'
    return buf, check


@pytest.fixture(autouse=True)
def _no_test_after_a_device_error():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:              # a sticky device error: nothing more may run on this device
        pytest.exit(f'device error, stopping: {e}', returncode=3)


def _bracket(got, ref, err):
    """elements outside round_bf16(ref - err) .. round_bf16(ref + err)"""
    lo, hi = conv_ref.round_bf16(ref - err), conv_ref.round_bf16(ref + err)
    return int(((got < lo) | (got > hi) | torch.isnan(got)).sum())


def _check_bf16(tag, got16, ref, r32, n_row, s_abs, ksplit):
    """both brackets of a bf16 result [rows, C] against float64 `ref`; prints the case's line"""
    got = got16.double()
    row_max = ref.abs().max(1, keepdim=True)[0].clamp(min=1e-300)
    e32 = float(((r32.double() - ref).abs() / row_max).max())
    ceil_err = (n_row[:, None].double() + ksplit) * U32 * s_abs
    work_err = max(1e-5, 4 * e32) * row_max.expand_as(ref)
    rb = conv_ref.round_bf16(ref)
    flip = got != rb
    share = float(flip.double().mean())
    mid = float((((ref - (rb + got) / 2).abs() / row_max)[flip]).max()) if bool(flip.any()) else 0.0
    over_c, over_w = _bracket(got, ref, ceil_err), _bracket(got, ref, work_err)
    print(f'{tag:44s} e32 {e32:.2e}  flips {share:.2e}  mid {mid:.2e}  outside ceiling {over_c}  working {over_w}')
    assert over_c == 0, f'{tag}: {over_c} elements outside the ceiling bracket (n + ksplit) 2^-24 S_abs'
    assert over_w == 0, f'{tag}: {over_w} elements outside the working bracket, e32 {e32:.3e}'


# ---------------------------------------------------------------------------------------------------
# forward: sg_spconv_gather_conv_bf16
# ---------------------------------------------------------------------------------------------------
def _run_bf16(lib, L, x, n_in, nbr, rows, K, cin, cout, w_k8, plan, ws_bytes):
    """one call into a NaN-filled output with poisoned spare rows, own workspace -> out [rows, cout] bf16"""
    out = torch.full((rows + SPARE, cout), float('nan'), dtype=torch.bfloat16, device=DEV)
    ws, check = _workspace(ws_bytes) if ws_bytes else (None, None)
    pl = (L.ptr(plan.order), L.ptr(plan.tile_mask), L.ptr(plan.nbr_tiles)) if plan is not None else (None, ) * 3
    L.check(lib.sg_spconv_gather_conv_bf16(L.ptr(x), n_in, L.ptr(nbr), rows, K, cin, cout, L.ptr(w_k8), *pl, L.ptr(out),
                                           L.ptr(ws), ws_bytes if ws is not None else 0, L.stream()),
            'sg_spconv_gather_conv_bf16')
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[rows:]).all()), 'rows behind the output written'
    if check is not None:
        check(core.conv_bf16_launch_info(rows, K, cin, cout, ws_bytes).ws_used)
    return out[:rows]


def _forward_both_ways(tag, x16, w, table, n_in, want, nows=None):
    """x16 [n_in, Cin] bf16, w [Cout, K, Cin] fp32 on the bf16 grid, table [rows, K] numpy: with and without plan
    (and without workspace where `nows` names that form) against float64"""
    from softgroup_amd import _lib as L
    lib = L.lib()
    rows, K = table.shape
    cout, cin = w.shape[0], w.shape[2]
    nbr = torch.from_numpy(np.ascontiguousarray(table)).to(DEV).contiguous()
    assert torch.equal(w.bfloat16().float(), w)
    w_k8 = core.pack_weight_bf16(w, cout, K, cin, False)
    ref = conv_ref.layer(x16.double(), w.double(), nbr)
    r32 = conv_ref.layer(x16.float(), w, nbr, dtype=torch.float32, bounds=False).out
    nb = lib.sg_spconv_conv_bf16_workspace_bytes(rows, cout)
    full = nb if nb > 256 else 0
    plan = core._Plan(nbr, rows, K)
    runs = [(full, want)] + ([(0, nows)] if nows is not None else [])
    for ws_bytes, form in runs:
        info = core.conv_bf16_launch_info(rows, K, cin, cout, ws_bytes)
        assert form is None or form_f(info) == form, f'{tag}: runs {form_f(info)}, named for {form}'
        for pl in (plan, None):
            what = f'{tag} {"plan" if pl is not None else "table"} ws={"yes" if ws_bytes else "no"} {form_f(info)}'
            out = _run_bf16(lib, L, x16, n_in, nbr, rows, K, cin, cout, w_k8, pl, ws_bytes)
            again = _run_bf16(lib, L, x16, n_in, nbr, rows, K, cin, cout, w_k8, pl, ws_bytes)
            assert torch.equal(out.view(torch.int16), again.view(torch.int16)), f'{what}: two runs differ'
            no_tap = ref.n == 0
            assert bool((out.view(torch.int16)[no_tap] == 0).all()), f'{what}: a row without a tap is not +0'
            _check_bf16(what, out, ref.out, r32, ref.n, ref.s_out, info.ksplit)
    return ref


@pytest.mark.parametrize('case', FCASES, ids=[c.name for c in FCASES])
def test_bf16_forward_against_float64(case):
    torch.cuda.set_device(0)
    K = KVOL[case.kind]
    table, n_in = tables(case.name, case.kind, case.rows, case.density)
    assert table.shape == (case.rows, K)
    gen = _gen(case.name)
    x16 = _vals((n_in, case.cin), gen).bfloat16().contiguous()
    w = _vals((case.cout, K, case.cin), gen).bfloat16().float()
    ref = _forward_both_ways(f'{case.name} K={K} {case.cin}->{case.cout} x {case.rows}', x16, w, table, n_in,
                             case.want, case.nows)
    if 'no_tap' in case.flags:
        assert bool((ref.n == 0).any())


# ---------------------------------------------------------------------------------------------------
# weight gradient: sg_spconv_wgrad
# ---------------------------------------------------------------------------------------------------
def _run_wgrad(lib, L, xa, ga, nbr_t, rows, K, cin, cout):
    dw = torch.full((K * cin + SPARE, cout), float('nan'), device=DEV)
    nb = lib.sg_spconv_wgrad_workspace_bytes(rows, K, cin, cout)
    ws, check = _workspace(nb)
    L.check(lib.sg_spconv_wgrad(L.ptr(xa), int(xa.dtype == torch.bfloat16), L.ptr(ga), int(ga.dtype == torch.bfloat16),
                                L.ptr(nbr_t), rows, K, cin, cout, L.ptr(dw), L.ptr(ws), nb, L.stream()), 'sg_spconv_wgrad')
    torch.cuda.synchronize()
    assert bool(torch.isnan(dw[K * cin:]).all()), 'rows behind the weight gradient written'
    check()
    return dw[:K * cin].view(K, cin, cout)


def _check_wgrad(tag, got, xa, ga, nbr):
    """both bars of a weight gradient [K, Cin, Cout] fp32 against conv_ref.wgrad on the operands as given"""
    K = nbr.shape[1]
    ref, s_abs, n = conv_ref.wgrad(xa.double(), ga.double(), nbr)
    worst, worst32, fails = 0.0, 0.0, []
    tl = nbr.long()
    for k in range(K):
        d = (got[k].double() - ref[k]).abs()
        if int(n[k]) == 0:
            assert bool((got[k] == 0).all()), f'{tag}: offset {k} has no pair and is not zero'
            continue
        j = torch.nonzero(tl[:, k] >= 0)[:, 0]
        r32 = xa.float()[tl[j, k]].t() @ ga.float()[j]
        scale = float(ref[k].abs().max())
        e32, err = float((r32.double() - ref[k]).abs().max()) / scale, float(d.max()) / scale
        worst, worst32 = max(worst, err), max(worst32, e32)
        over = float((d - (float(n[k]) + 8) * U32 * s_abs[k]).max())
        if over > 0 or not err <= max(1e-5, 4 * e32):
            fails.append((k, int(n[k]), err, e32, over))
    print(f'{tag:52s} err {worst:.2e}  e32 {worst32:.2e}')
    assert not fails, f'{tag}: (offset, pairs, error / max|ref|, e32, above the ceiling) {fails}'


@pytest.mark.parametrize('case', WCASES, ids=[c.name for c in WCASES])
def test_wgrad_against_float64(case):
    from softgroup_amd import _lib as L
    lib = L.lib()
    torch.cuda.set_device(0)
    K = KVOL[case.kind]
    table, n_in = tables(case.name, case.kind, case.rows)
    info = core.wgrad_launch_info(case.rows, K, case.cin, case.cout)
    assert form_w(info) == case.want, f'{case.name}: runs {form_w(info)}, named for {case.want}'
    nbr = torch.from_numpy(np.ascontiguousarray(table)).to(DEV).contiguous()
    nbr_t = nbr.t().contiguous()                        # [K, M] by torch, not by the library's transpose
    gen = _gen(case.name)
    x, g = _vals((n_in, case.cin), gen), _vals((case.rows, case.cout), gen)
    for ta, tg in case.types:
        xa = (x.bfloat16() if ta else x).contiguous()
        ga = (g.bfloat16() if tg else g).contiguous()
        got = _run_wgrad(lib, L, xa, ga, nbr_t, case.rows, K, case.cin, case.cout)
        again = _run_wgrad(lib, L, xa, ga, nbr_t, case.rows, K, case.cin, case.cout)
        assert torch.equal(got, again), f'{case.name}: two runs differ'
        tag = (f'{case.name} K={K} {case.cin}->{case.cout} x {case.rows} {"bf16" if ta else "fp32"}/'
               f'{"bf16" if tg else "fp32"} {form_w(info)}')
        _check_wgrad(tag, got, xa, ga, nbr)


# ---------------------------------------------------------------------------------------------------
# the modules under bf16 autocast: input gradient (transposed table, packed(True, True)) and weight gradient
# ---------------------------------------------------------------------------------------------------
def _keys(idx, shape):
    idx = idx.long()
    return ((idx[:, 0] * shape[0] + idx[:, 1]) * shape[1] + idx[:, 2]) * shape[2] + idx[:, 3]


@pytest.mark.parametrize('kind,cin,cout', MCASES, ids=[f'{k}_{a}_{b}' for k, a, b in MCASES])
def test_module_gradients_under_autocast_against_float64(kind, cin, cout):
    import softgroup_amd.spconv.pytorch as spconv
    torch.cuda.set_device(0)
    name = f'module_{kind}_{cin}_{cout}'
    rng = _rng(name)
    ext = G._extent(MROWS / 0.4)                       # odd extents: the inverse conv has rows without a tap
    idx = exact_voxels(rng, MROWS, ext, 1)
    ti = torch.from_numpy(idx).to(DEV)
    gen = _gen(name)
    K = KVOL[kind]
    if kind == 'subm':
        table, n_in, n_out = conv_ref.subm_table(idx, ext), MROWS, MROWS
        mod = spconv.SubMConv3d(cin, cout, 3, padding=1, bias=False, indice_key='s').to(DEV)
        in_perm = out_perm = None
    else:
        child, up, m_par = conv_ref.down_tables(idx, ext)
        # rows of the coarse level: the oracle's order against the library's, matched by coordinate
        first = np.where(child >= 0, child, len(idx)).min(1)
        par = np.concatenate([idx[first, :1], idx[first, 1:] >> 1], 1)
        down = spconv.SparseConv3d(cin if kind == 'down' else cout, cout if kind == 'down' else cin, kernel_size=2,
                                   stride=2, bias=False, indice_key='d').to(DEV)
        with torch.no_grad():
            probe = down(spconv.SparseConvTensor(torch.zeros(MROWS, down.in_channels, device=DEV), ti, ext, 1))
        cshape = [e // 2 for e in ext]
        assert probe.indices.shape[0] == m_par
        ko = _keys(torch.from_numpy(par).to(DEV), cshape)
        kl = _keys(probe.indices, cshape)
        so, sl = torch.argsort(ko), torch.argsort(kl)
        assert torch.equal(ko[so], kl[sl])
        perm = torch.empty_like(so)
        perm[sl] = so                                  # library row i is oracle row perm[i]
        if kind == 'down':
            table, n_in, n_out, mod, in_perm, out_perm = child, MROWS, m_par, down, None, perm
        else:
            table, n_in, n_out, in_perm, out_perm = up, m_par, MROWS, perm, None
            mod = spconv.SparseInverseConv3d(cin, cout, kernel_size=2, bias=False, indice_key='d').to(DEV)
    with torch.no_grad():
        mod.weight.copy_(_vals(tuple(mod.weight.shape), gen))
    x = _vals((n_in, cin), gen)                        # oracle row order
    r = _vals((n_out, cout), gen).bfloat16().float()   # the gradient of the output, on the bf16 grid
    feats = (x if in_perm is None else x[in_perm]).clone().requires_grad_(True)
    r_lib = r if out_perm is None else r[out_perm]

    def run():
        feats.grad = mod.weight.grad = None
        with torch.autocast('cuda', dtype=torch.bfloat16):
            if kind == 'up':
                inp = probe.replace_feature(feats)
            else:
                inp = spconv.SparseConvTensor(feats, ti, ext, 1)
            y = mod(inp)
        assert y.features.dtype == torch.bfloat16 and y.features.shape == (n_out, cout)
        (y.features.float() * r_lib).sum().backward()
        return feats.grad.clone(), mod.weight.grad.clone()

    dx, dw = run()
    dx2, dw2 = run()
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2), 'two runs differ'
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dw).all())
    nbr = torch.from_numpy(np.ascontiguousarray(table)).to(DEV)
    w16 = mod.weight.detach().reshape(cout, K, cin).bfloat16()
    x16, g16 = x.bfloat16(), r.bfloat16()
    # input gradient: a bf16 tensor behind the autocast cast, rows back in the oracle's order
    ref, s_abs, n = conv_ref.input_grad(g16.double(), w16.double(), nbr, n_in)
    r32 = torch.zeros(n_in, cin, device=DEV)
    tl = nbr.long()
    for k in range(K):
        j = torch.nonzero(tl[:, k] >= 0)[:, 0]
        r32.index_add_(0, tl[j, k], g16.float()[j] @ w16.float()[:, k, :])
    got = dx.detach()
    if in_perm is not None:
        got = torch.empty_like(got).index_copy_(0, in_perm, got)
    assert torch.equal(got.bfloat16().float(), got), 'the input gradient is not on the bf16 grid'
    info = core.conv_bf16_launch_info(n_in, K, cout, cin)
    _check_bf16(f'{name} dgrad {form_f(info)}', got.bfloat16(), ref, r32, n, s_abs, info.ksplit)
    # weight gradient, in the parameter's layout [Cout, k, k, k, Cin]
    _check_wgrad(f'{name} wgrad {form_w(core.wgrad_launch_info(n_out, K, cin, cout))}',
                 dw.reshape(cout, K, cin).permute(1, 2, 0).contiguous(), x16, g16, nbr)


# ---------------------------------------------------------------------------------------------------
# sg_spconv_pack_weight_bf16
# ---------------------------------------------------------------------------------------------------
# float32 bit patterns: ties between two bf16 values (both parities, both signs), one bit off a tie, the largest
# finite float (rounds to inf), +-inf, three NaNs (quiet, negative with payload, signalling), subnormals
SPECIAL_BITS = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0x7F800000,
                0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x00000001, 0x80008000]


@pytest.mark.parametrize('cin', [6, 7, 20, 32])
@pytest.mark.parametrize('src_kio', [0, 1])
def test_pack_weight_bf16_bits_and_padding(cin, src_kio):
    from softgroup_amd import _lib as L
    lib = L.lib()
    torch.cuda.set_device(0)
    K, cout = 8, 33
    gen = _gen(f'pack_{cin}_{src_kio}')
    w = torch.randn(cout, K, cin, device=DEV, generator=gen)                 # logical [Cout][K][Cin]
    flat = w.view(-1)
    # ties (halfway between two bf16 values, both parities and signs), +-inf, NaN
    special = torch.from_numpy(np.array(SPECIAL_BITS, np.uint32).view(np.float32).copy()).to(DEV)
    at = torch.randperm(flat.numel(), device=DEV, generator=gen)[:special.numel()]
    flat[at] = special
    src = (w.permute(1, 2, 0) if src_kio else w).contiguous()
    n = lib.sg_spconv_packed_weight_elems_bf16(K, cin, cout)
    c8p = (cin + 15) // 16 * 2
    assert n == K * c8p * cout * 8
    out = torch.full((n + SPARE, ), float('nan'), dtype=torch.bfloat16, device=DEV)
    L.check(lib.sg_spconv_pack_weight_bf16(L.ptr(src), cout, K, cin, src_kio, L.ptr(out), L.stream()),
            'sg_spconv_pack_weight_bf16')
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[n:]).all())
    got = out[:n].view(K, c8p, cout, 8).permute(2, 0, 1, 3).reshape(cout, K, c8p * 8)      # [Cout][K][padded Cin]
    real, pad = got[:, :, :cin], got[:, :, cin:]
    assert bool((pad.contiguous().view(torch.int16) == 0).all()), 'a padding entry is not +0'
    want = w.bfloat16()
    nan = torch.isnan(w)
    assert bool(torch.isnan(real[nan]).all()) and int(nan.sum()) == 3
    assert torch.equal(real.contiguous().view(torch.int16)[~nan], want.contiguous().view(torch.int16)[~nan])
    # ... and torch's conversion is the single rounding of the reference
    fin = torch.isfinite(w)
    assert torch.equal(conv_ref.round_bf16(w.double())[fin], want.double()[fin])
