// nms_greedy.h -- the two order-dependent kernels of greedy NMS, for callers outside mask_nms.hip (box_ops.hip).
// The kernels live in mask_nms.hip, which launches them itself for sg_mask_nms; these host functions launch the
// same kernels on the caller's arrays and stream.  Nothing synchronises; the caller checks the launch.
#pragma once
#include "common.h"

namespace sg {

// rank[i] = items visited before item i (descending score, the LOWER index first among equal scores; -0.0 == 0.0),
// order[rank[i]] = i.  scores float32 [n], rank / order int32 [n], 0 <= n <= 16384.
void nms_rank_launch(const float *scores, int n, int32_t *rank, int32_t *order, hipStream_t stream);

// decide uint32 [n, nw], nw = ceil(n / 32), indexed by rank: bit r2 of row r1 < r2 = the item of rank r1, when kept,
// suppresses the item of rank r2.  One wave walks the ranks.  keep uint8 [n] in original indices, *n_keep their number.
// 0 <= n <= 16384 (the `removed` vector is in LDS).
void nms_greedy_launch(const uint32_t *decide, const int32_t *order, int n, int nw, uint8_t *keep, int32_t *n_keep,
                       hipStream_t stream);

}  // namespace sg
