// cross_links.h -- the rectangular intersection / link kernel of stitch.hip, shared with ensemble.hip: one kernel,
// one decision.  sg_mask_cross_links runs it on the rows of two tiles, sg_mask_group_links on one stacked matrix
// against itself with a group number per row.
#pragma once
#include "common.h"

namespace sg {

constexpr int kClTile = 4;

struct ClArgs {
  const uint32_t *bits_a, *bits_b;
  const int32_t *labels_a, *labels_b;
  const int32_t *group_a, *group_b;      // null, or a group per row: rows of equal groups are never linked
  uint32_t *adj;                         // [n_total, nw] symmetric
  int32_t *inter_out, *cnt_a_out, *cnt_b_out;
  double thr;
  int64_t n_bits, words;
  int n_a, n_b, base_a, base_b, n_total, nw, measure, min_shared;
  int symmetric;                         // a and b are the same rows: tile pairs below the diagonal are skipped
};

// launches cross_links_kernel over the ceil(n_a / 4) x ceil(n_b / 4) tile pairs, at most max_blocks workgroups
void cross_links_launch(const ClArgs &a, int max_blocks, hipStream_t stream);

}  // namespace sg
