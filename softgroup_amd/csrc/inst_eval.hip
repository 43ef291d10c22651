// inst_eval.hip -- ScanNetEval on the device (softgroup/evaluation/instance_eval.py): RLE text -> runs
// -> GT instance table -> intersections -> IoU pair records -> greedy matching -> sorted PR curves ->
// ap / rc [n_labels, n_thresholds].  The host evaluator (softgroup_amd/evaluation/instance_eval.py) is the
// specification; every stage below cites the reference lines it replaces.
//
//   sg_inst_rle_parse   one workgroup per mask: token starts by a block scan over the bytes, every token
//                       start parses its own number; then the mask's runs are range-checked and summed
//   sg_inst_scan_update one scan: GT ids are class * 1000 + instance, so the evaluated ones lie in
//                       n_classes * 1000 bins -- a histogram, compacted in bin order, IS np.unique's
//                       ascending table; a thread per mask point adds to counts[pred, slot]; the non-zero
//                       same-label entries become pair records in both orders the matcher walks; one
//                       thread per (label, threshold) of this scan does the greedy walk twice (count,
//                       then emit at scanned offsets) and appends (score key, segment, true flag)
//                       examples to the evaluation's accumulator.  The walk is sequential only inside one
//                       (scan, label, threshold): the reference's `visited` keys carry the scan id.
//   sg_inst_scan_coverage  (opt-in) the S3DIS columns from the same pair records: per label the best IoU of
//                       every GT and of every prediction, coverage sums in ascending GT order, tp / fp tallies
//   sg_inst_curves      examples ordered by (segment, score key) with three stable LSD radix sorts, then a
//                       workgroup per (label, threshold): cumulative true count, unique score boundaries,
//                       precision / recall in double, AP summed in a fixed order.
// Integer arithmetic and comparisons only until the quotients; no floating-point atomics: results are
// bitwise repeatable.  Every list walk is bounded by its table entry and by the capacity of its buffer.
#include "common.h"
#include "radix_sort.h"
#include "scan.h"

namespace sg {

constexpr int kIeBlock = 256;
constexpr int kIeBinsPerClass = 1000;          // gt id = class * 1000 + instance (instance_eval.py:235)

__device__ __forceinline__ bool ie_is_space(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); }
__device__ __forceinline__ bool ie_is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// first run slot of mask m: a run takes at least 4 bytes of text ("s l" + separator, the last mask's
// separator paid by the + m), so the masks' slot ranges never overlap
__host__ __device__ __forceinline__ int64_t ie_slot_base(int64_t text_off, int64_t m) { return (text_off + m) / 4; }

// ---- 1. RLE text -> runs (rle_decode's split, util/rle.py; instance_eval.py:377) ---------------------
__global__ void __launch_bounds__(kIeBlock) ie_parse_kernel(
    const uint8_t *__restrict__ text, const int64_t *__restrict__ text_off, const int32_t *__restrict__ mask_pred,
    int64_t text_bytes, int64_t length, int32_t *__restrict__ run_start, int32_t *__restrict__ run_len,
    int32_t *__restrict__ run_pred, int64_t run_slots, int32_t *__restrict__ vert_count,
    int32_t *__restrict__ flags) {
  __shared__ int lds4[4];
  __shared__ long long red[kIeBlock];
  const int m = blockIdx.x, tid = threadIdx.x;
  int64_t b0 = text_off[m], b1 = text_off[m + 1];
  int32_t bad = 0;
  if (b0 < 0 || b1 < b0 || b1 > text_bytes) {          // a broken offset table reads nothing
    bad |= SG_INST_BAD_TEXT;
    b0 = b1 = 0;
  }
  const int pred = mask_pred ? mask_pred[m] : m;
  int64_t s0 = ie_slot_base(b0, m), s1 = ie_slot_base(b1, m + 1);
  if (s1 > run_slots || m == static_cast<int>(gridDim.x) - 1) s1 = run_slots;   // the last mask owns the spare slots
  if (s0 > s1) s0 = s1;
  for (int64_t s = s0 + tid; s < s1; s += kIeBlock) {
    run_start[s] = 0;
    run_len[s] = 0;
    run_pred[s] = pred;
  }
  __syncthreads();
  int carry = 0;                                        // tokens before this chunk
  for (int64_t c0 = b0; c0 < b1; c0 += kIeBlock) {      // (uniform bounds: every thread takes every round)
    const int64_t i = c0 + tid;
    bool start = false;
    if (i < b1) {
      const uint8_t c = text[i];
      const bool d = ie_is_digit(c);
      if (!d && !ie_is_space(c)) bad |= SG_INST_BAD_TEXT;
      start = d && (i == b0 || !ie_is_digit(text[i - 1]));
    }
    int total = 0;
    const int incl = block_incl_scan_256(start ? 1 : 0, lds4, &total);
    if (start) {
      const int t = carry + incl - 1;
      int64_t v = 0;
      int nd = 0;
      for (int64_t j = i; j < b1 && ie_is_digit(text[j]); ++j, ++nd)
        if (nd < 12) v = v * 10 + (text[j] - '0');
      if (nd >= 12 || v > 0x7fffffffLL) {
        bad |= SG_INST_RUN_RANGE;
        v = 0x7fffffffLL;
      }
      const int64_t s = s0 + (t >> 1);
      if (s < s1) {
        if (t & 1) run_len[s] = static_cast<int32_t>(v);
        else run_start[s] = static_cast<int32_t>(v - 1);      // 1-based in the text
      }
    }
    carry += total;
  }
  if (carry & 1) bad |= SG_INST_ODD_TOKENS;
  __syncthreads();
  // range check; a run that fails it is emptied so that no later stage indexes past the scan
  const int n_runs = carry >> 1;
  long long sum = 0;
  for (int r = tid; r < n_runs; r += kIeBlock) {
    const int64_t s = s0 + r;
    if (s >= s1) break;
    const int64_t a = run_start[s], l = run_len[s];
    if (a < 0 || l < 0 || a + l > length) {
      bad |= SG_INST_RUN_RANGE;
      run_start[s] = 0;
      run_len[s] = 0;
    } else {
      sum += l;
    }
  }
  red[tid] = sum;
  __syncthreads();
  for (int s = kIeBlock / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const long long vert = red[0];
  if (vert > length) {                                  // overlapping runs: more mask points than points
    bad |= SG_INST_RUN_RANGE;
    for (int64_t s = s0 + tid; s < s1; s += kIeBlock) run_len[s] = 0;
  }
  if (tid == 0) vert_count[pred] = vert > length ? 0 : static_cast<int32_t>(vert);
  if (bad) atomicOr(flags, bad);
}

// ---- 2. association (get_instances, instance_eval_util.py; assign_instances_for_scan :228-309) ------
// per-scan tables inside the workspace
struct IeScan {
  uint32_t *hist;        // [n_bins] points per evaluated gt id
  int32_t *counts;       // [n_pred][gt_cap + 1], column gt_cap = void
  uint8_t *visited;      // [2][n_thr][n_pred] (count walk, emit walk)
  int32_t *info;         // [8]: 0 n_gt, 1 total mask points, 2 n_pairs
  int32_t *bin_slot;     // [n_bins]
  int32_t *run_off;      // [run_slots + 1]
  int32_t *gt_id, *gt_label, *gt_vert;      // [gt_cap]
  int32_t *gt_pair_off;  // [gt_cap + 1]
  int32_t *pred_pair_off;   // [n_pred + 1]
  int32_t *pred_void;    // [n_pred]
  int32_t *pa_gt, *pa_pred, *pa_inter;      // pairs by gt, then prediction   [pair_cap]
  double *pa_iou;
  int32_t *pb_gt, *pb_pred, *pb_inter;      // pairs by prediction, then gt
  double *pb_iou;
  int32_t *item_cnt;     // [n_items]
  void *scan_ws;
  size_t scan_ws_bytes;
  size_t zero_bytes;     // hist .. info are one region, zeroed per scan
  int n_bins, gt_cap, n_pred;
  int64_t pair_cap, run_slots;
};

static bool ie_carve(void *ws, size_t ws_bytes, int n_pred, int64_t run_slots, int n_classes, int gt_cap,
                     int n_thr, int n_labels, IeScan *t, size_t *used, int64_t *offs) {
  Workspace w(ws, ws_bytes);
  t->n_bins = n_classes * kIeBinsPerClass;
  t->gt_cap = gt_cap;
  t->n_pred = n_pred;
  t->run_slots = run_slots;
  t->pair_cap = static_cast<int64_t>(n_pred) * gt_cap;
  const size_t np = static_cast<size_t>(n_pred), pc = static_cast<size_t>(t->pair_cap);
  t->hist = w.take<uint32_t>(t->n_bins);
  t->counts = w.take<int32_t>(np * (gt_cap + 1) + 1);
  t->visited = w.take<uint8_t>(2 * np * n_thr + 1);
  t->info = w.take<int32_t>(8);
  t->zero_bytes = w.off;
  t->bin_slot = w.take<int32_t>(t->n_bins);
  t->run_off = w.take<int32_t>(run_slots + 1);
  t->gt_id = w.take<int32_t>(gt_cap);
  t->gt_label = w.take<int32_t>(gt_cap);
  t->gt_vert = w.take<int32_t>(gt_cap);
  t->gt_pair_off = w.take<int32_t>(gt_cap + 1);
  t->pred_pair_off = w.take<int32_t>(np + 1);
  t->pred_void = w.take<int32_t>(np + 1);
  t->pa_gt = w.take<int32_t>(pc + 1);
  t->pa_pred = w.take<int32_t>(pc + 1);
  t->pa_inter = w.take<int32_t>(pc + 1);
  t->pa_iou = w.take<double>(pc + 1);
  t->pb_gt = w.take<int32_t>(pc + 1);
  t->pb_pred = w.take<int32_t>(pc + 1);
  t->pb_inter = w.take<int32_t>(pc + 1);
  t->pb_iou = w.take<double>(pc + 1);
  t->item_cnt = w.take<int32_t>(static_cast<size_t>(n_labels) * n_thr);
  t->scan_ws_bytes = scan_workspace_bytes(run_slots + 1);
  t->scan_ws = w.take<char>(t->scan_ws_bytes);
  if (used) *used = w.off;
  if (offs) {
    char *b = static_cast<char *>(ws);
    const void *sec[SG_INST_SECTIONS] = {t->info, t->gt_id, t->gt_label, t->gt_vert, t->gt_pair_off, t->pred_pair_off,
                                         t->pred_void, t->pa_gt, t->pa_pred, t->pa_inter, t->pa_iou, t->pb_gt,
                                         t->pb_pred, t->pb_inter, t->pb_iou, t->counts};
    for (int i = 0; i < SG_INST_SECTIONS; ++i) offs[i] = static_cast<const char *>(sec[i]) - b;
  }
  return t->scan_ws != nullptr;
}

// points per evaluated gt id; one atomic per distinct id of a wave (a scan's points are ordered in space)
__global__ void __launch_bounds__(kIeBlock) ie_gt_hist_kernel(const int64_t *__restrict__ gts, int64_t n,
                                                              int n_bins, uint32_t *__restrict__ hist,
                                                              int32_t *__restrict__ flags) {
  const int lane = threadIdx.x & 63;
  int32_t bad = 0;
  for (int64_t i0 = (blockIdx.x * static_cast<int64_t>(kIeBlock) + threadIdx.x) - lane; i0 < n;
       i0 += static_cast<int64_t>(gridDim.x) * kIeBlock) {
    const int64_t i = i0 + lane;
    int bin = -1;
    if (i < n) {
      const int64_t id = gts[i];
      if (id < 0 || id >= (1LL << 31)) bad |= SG_INST_BAD_GT;
      else if (id >= kIeBinsPerClass && id - kIeBinsPerClass < n_bins) bin = static_cast<int>(id - kIeBinsPerClass);
    }
    uint64_t todo = __ballot(bin >= 0);
    while (todo) {
      const int leader = __ffsll(static_cast<long long>(todo)) - 1;
      const int b = __shfl(bin, leader, 64);
      const uint64_t same = __ballot(bin == b) & todo;
      if (lane == leader) atomicAdd(&hist[b], static_cast<uint32_t>(__popcll(same)));
      todo &= ~same;
    }
  }
  if (bad) atomicOr(flags, bad);
}

// the non-empty bins in ascending id = np.unique's order, ids of evaluated classes only
__global__ void __launch_bounds__(kIeBlock) ie_gt_table_kernel(IeScan t, int agnostic, int32_t *__restrict__ flags) {
  __shared__ int lds4[4];
  constexpr int kItems = 8;
  int carry = 0;
  for (int c0 = 0; c0 < t.n_bins; c0 += kIeBlock * kItems) {
    const int first = c0 + threadIdx.x * kItems;
    uint32_t h[kItems];
    int mine = 0;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      h[k] = first + k < t.n_bins ? t.hist[first + k] : 0u;
      mine += h[k] ? 1 : 0;
    }
    int total = 0;
    int slot = carry + block_incl_scan_256(mine, lds4, &total) - mine;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const int b = first + k;
      if (b >= t.n_bins) break;
      int s = t.gt_cap;                                  // void
      if (h[k]) {
        if (slot < t.gt_cap) {
          s = slot;
          t.gt_id[slot] = b + kIeBinsPerClass;
          t.gt_label[slot] = agnostic ? 0 : b / kIeBinsPerClass;
          t.gt_vert[slot] = static_cast<int32_t>(h[k]);
        }
        ++slot;
      }
      t.bin_slot[b] = s;
    }
    carry += total;
  }
  if (threadIdx.x == 0) {
    t.info[0] = carry < t.gt_cap ? carry : t.gt_cap;
    if (carry > t.gt_cap) atomicOr(flags, SG_INST_OVERFLOW_GT);
  }
}

// eval_intersections_kernel (eval_ops.hip) with the slot looked up from the gt id and the number of mask
// points read from the device (the runs were parsed there)
__global__ void __launch_bounds__(kIeBlock) ie_intersections_kernel(
    const int32_t *__restrict__ run_start, const int32_t *__restrict__ run_pred, const int64_t *__restrict__ gts,
    int64_t n_points, IeScan t) {
  const int lane = threadIdx.x & 63;
  const int64_t total = t.info[1];
  const int n_runs = static_cast<int>(t.run_slots);
  const int stride = t.gt_cap + 1;
  for (int64_t t0 = (blockIdx.x * static_cast<int64_t>(kIeBlock) + threadIdx.x) - lane; t0 < total;
       t0 += static_cast<int64_t>(gridDim.x) * kIeBlock) {
    const int64_t q = t0 + lane;
    bool valid = q < total;
    int key = -1;
    if (valid) {
      int lo = 0, hi = n_runs;                           // last run with run_off[r] <= q
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t.run_off[mid] <= q) lo = mid; else hi = mid;
      }
      const int64_t point = run_start[lo] + (q - t.run_off[lo]);
      const int p = run_pred[lo];
      valid = point >= 0 && point < n_points && p >= 0 && p < t.n_pred;
      if (valid) {
        const int64_t id = gts[point];
        int slot = t.gt_cap;
        if (id >= kIeBinsPerClass && id - kIeBinsPerClass < t.n_bins) slot = t.bin_slot[id - kIeBinsPerClass];
        key = p * stride + slot;
      }
    }
    uint64_t todo = __ballot(valid);
    while (todo) {
      const int leader = __ffsll(static_cast<long long>(todo)) - 1;
      const int k = __shfl(key, leader, 64);
      const uint64_t same = __ballot(valid && key == k) & todo;
      if (lane == leader) atomicAdd(&t.counts[k], __popcll(same));
      todo &= ~same;
    }
  }
}

struct IePreds {
  const int32_t *label;   // evaluated label index, -1: not evaluated
  const int32_t *vert;
  const double *conf;
  int64_t min_region;
};
__device__ __forceinline__ bool ie_kept(const IePreds &p, int i) {
  return p.label[i] >= 0 && p.vert[i] >= p.min_region;        // instance_eval.py:262-271
}

// pair records: same label and intersection > 0 (:290-305), iou = float(inter) / (gt + pred - inter)
__global__ void __launch_bounds__(kIeBlock) ie_pairs_kernel(IeScan t, IePreds pr) {
  __shared__ int lds4[4];
  const int n_gt = t.info[0], n_pred = t.n_pred, stride = t.gt_cap + 1;
  // by prediction, then gt
  int carry = 0;
  for (int c0 = 0; c0 < n_pred; c0 += kIeBlock) {
    const int p = c0 + threadIdx.x;
    int cnt = 0;
    const bool on = p < n_pred && ie_kept(pr, p);
    if (on) {
      const int lab = pr.label[p];
      for (int g = 0; g < n_gt; ++g) cnt += (t.gt_label[g] == lab && t.counts[p * stride + g] > 0) ? 1 : 0;
    }
    int total = 0;
    int q = carry + block_incl_scan_256(cnt, lds4, &total) - cnt;
    if (p < n_pred) {
      t.pred_pair_off[p] = q;
      t.pred_void[p] = t.counts[p * stride + t.gt_cap];
    }
    if (on) {
      const int lab = pr.label[p], pv = pr.vert[p];
      for (int g = 0; g < n_gt; ++g) {
        const int inter = t.counts[p * stride + g];
        if (t.gt_label[g] != lab || inter <= 0) continue;
        if (q < t.pair_cap) {
          t.pb_gt[q] = g;
          t.pb_pred[q] = p;
          t.pb_inter[q] = inter;
          t.pb_iou[q] = static_cast<double>(inter) /
                        static_cast<double>(static_cast<int64_t>(t.gt_vert[g]) + pv - inter);
        }
        ++q;
      }
    }
    carry += total;
  }
  if (threadIdx.x == 0) {
    t.pred_pair_off[n_pred] = carry;
    t.info[2] = carry;
  }
  // by gt, then prediction
  carry = 0;
  for (int c0 = 0; c0 < n_gt; c0 += kIeBlock) {
    const int g = c0 + threadIdx.x;
    int cnt = 0;
    if (g < n_gt) {
      const int lab = t.gt_label[g];
      for (int p = 0; p < n_pred; ++p)
        cnt += (ie_kept(pr, p) && pr.label[p] == lab && t.counts[p * stride + g] > 0) ? 1 : 0;
    }
    int total = 0;
    int q = carry + block_incl_scan_256(cnt, lds4, &total) - cnt;
    if (g < n_gt) {
      t.gt_pair_off[g] = q;
      const int lab = t.gt_label[g], gv = t.gt_vert[g];
      for (int p = 0; p < n_pred; ++p) {
        if (!ie_kept(pr, p) || pr.label[p] != lab) continue;
        const int inter = t.counts[p * stride + g];
        if (inter <= 0) continue;
        if (q < t.pair_cap) {
          t.pa_gt[q] = g;
          t.pa_pred[q] = p;
          t.pa_inter[q] = inter;
          t.pa_iou[q] = static_cast<double>(inter) / static_cast<double>(static_cast<int64_t>(gv) + pr.vert[p] - inter);
        }
        ++q;
      }
    }
    carry += total;
  }
  if (threadIdx.x == 0) t.gt_pair_off[n_gt] = carry;
}

// ---- 3. matching (evaluate_matches :82-139) ------------------------------------------------------------
struct IeThr {
  double v[SG_INST_MAX_THRESHOLDS];
  int n;
};
struct IeAcc {
  uint64_t *ex_key;
  uint32_t *ex_meta;      // segment << 1 | true flag
  int64_t ex_cap;
  int32_t *seg_stats;     // [4][n_seg]: examples, hard false negatives, has_gt, has_pred
  int64_t *totals;        // [0] examples appended so far (counted past the capacity too)
  int32_t *flags;
};

// order-preserving key of a finite double (no NaN reaches here; -0.0 was canonicalised by the caller)
__device__ __forceinline__ uint64_t ie_score_key(double d) {
  const uint64_t b = static_cast<uint64_t>(__double_as_longlong(d));
  return (b >> 63) ? ~b : (b | (1ULL << 63));
}

// one (label, threshold) of the scan.  out < 0: count only.  Returns the number of examples.
__device__ int ie_walk(const IeScan &t, const IePreds &pr, int label, double th, uint8_t *visited, int64_t out,
                       const IeAcc &acc, uint32_t seg, int *hard_fn_out, int *has_gt_out, int *has_pred_out) {
  const int n_gt = t.info[0], n_pred = t.n_pred;
  const int n_pairs = t.info[2] < t.pair_cap ? t.info[2] : static_cast<int>(t.pair_cap);
  int n_ex = 0, hard_fn = 0, has_gt = 0, has_pred = 0;
  auto emit = [&](double score, uint32_t is_true) {
    if (out >= 0 && out + n_ex < acc.ex_cap) {
      acc.ex_key[out + n_ex] = ie_score_key(score);
      acc.ex_meta[out + n_ex] = seg << 1 | is_true;
    }
    ++n_ex;
  };
  for (int g = 0; g < n_gt; ++g) {                       // list order = ascending id
    if (t.gt_label[g] != label || t.gt_vert[g] < pr.min_region) continue;
    has_gt = 1;
    bool matched = false;
    double score = 0.0;
    int q0 = t.gt_pair_off[g], q1 = t.gt_pair_off[g + 1];
    if (q0 < 0) q0 = 0;
    if (q1 > n_pairs) q1 = n_pairs;
    for (int q = q0; q < q1; ++q) {                      // prediction order
      const int p = t.pa_pred[q];
      if (p < 0 || p >= n_pred || visited[p]) continue;
      if (t.pa_iou[q] > th) {
        const double conf = pr.conf[p];
        if (matched) {                                   // the lower score is a false positive; p stays unvisited
          const double hi = score > conf ? score : conf, lo = score > conf ? conf : score;
          score = hi;
          emit(lo, 0u);
        } else {
          matched = true;
          score = conf;
          visited[p] = 1;
        }
      }
    }
    if (matched) emit(score, 1u);
    else ++hard_fn;
  }
  for (int p = 0; p < n_pred; ++p) {                     // :116-139
    if (!ie_kept(pr, p) || pr.label[p] != label) continue;
    has_pred = 1;
    bool any = false;
    int64_t ignore = t.pred_void[p];
    int q0 = t.pred_pair_off[p], q1 = t.pred_pair_off[p + 1];
    if (q0 < 0) q0 = 0;
    if (q1 > n_pairs) q1 = n_pairs;
    for (int q = q0; q < q1; ++q) {
      if (t.pb_iou[q] > th) any = true;
      const int g = t.pb_gt[q];
      if (g >= 0 && g < n_gt && t.gt_vert[g] < pr.min_region) ignore += t.pb_inter[q];
    }
    if (any) continue;
    if (static_cast<double>(ignore) / static_cast<double>(pr.vert[p]) <= th) emit(pr.conf[p], 0u);
  }
  *hard_fn_out = hard_fn;
  *has_gt_out = has_gt;
  *has_pred_out = has_pred;
  return n_ex;
}

__global__ void __launch_bounds__(kIeBlock) ie_match_kernel(IeScan t, IePreds pr, IeThr thr, int n_labels, IeAcc acc) {
  __shared__ int lds4[4];
  const int n_items = n_labels * thr.n;
  const int64_t base = acc.totals[0];
  int hf, hg, hp;
  for (int c0 = 0; c0 < n_items; c0 += kIeBlock) {       // count walk
    const int it = c0 + threadIdx.x;
    if (it < n_items) {
      const int oi = it % thr.n;
      t.item_cnt[it] = ie_walk(t, pr, it / thr.n, thr.v[oi], t.visited + static_cast<size_t>(oi) * t.n_pred, -1, acc,
                               0u, &hf, &hg, &hp);
    }
  }
  __syncthreads();
  int carry = 0;
  for (int c0 = 0; c0 < n_items; c0 += kIeBlock) {       // offsets in item order, emit walk
    const int it = c0 + threadIdx.x;
    const int cnt = it < n_items ? t.item_cnt[it] : 0;
    int total = 0;
    const int excl = carry + block_incl_scan_256(cnt, lds4, &total) - cnt;
    if (it < n_items) {
      const int oi = it % thr.n;
      const int64_t out = base + excl;
      if (out + cnt > acc.ex_cap) atomicOr(acc.flags, SG_INST_OVERFLOW_EX);
      ie_walk(t, pr, it / thr.n, thr.v[oi], t.visited + static_cast<size_t>(thr.n + oi) * t.n_pred, out, acc,
              static_cast<uint32_t>(it), &hf, &hg, &hp);
      // scans follow each other on the stream and an item is one thread's: plain updates
      acc.seg_stats[it] += cnt;
      acc.seg_stats[n_items + it] += hf;
      acc.seg_stats[2 * n_items + it] |= hg;
      acc.seg_stats[3 * n_items + it] |= hp;
    }
    carry += total;
  }
  if (threadIdx.x == 0) acc.totals[0] = base + carry;
}

// ---- 3b. coverage, precision and recall of the scan (S3DIS tables; no reference code, softgroup_hip.h
// states the definitions) -------------------------------------------------------------------------------
struct IeCov {
  double iou_thr, score_thr;
  double *sums;            // [2][n_labels]: cov, wcov summed over the rooms
  int64_t *tallies;        // [5][n_labels]: rooms, n_gt, gt_hit, tp, fp
  const int32_t *flags;
  int n_labels;
};

// one workgroup per label.  The maxima are order-free: a thread per prediction, then a thread per GT row,
// kIeBlock rows at a time; thread 0 adds each batch in ascending row (= id) order, so the sums are the
// host's, bit for bit.
__global__ void __launch_bounds__(kIeBlock) ie_coverage_kernel(IeScan t, IePreds pr, IeCov c) {
  __shared__ double ov_s[kIeBlock];
  __shared__ int32_t vert_s[kIeBlock];
  __shared__ uint8_t on_s[kIeBlock];
  __shared__ int cnt_s[2];
  if (*c.flags) return;                                  // (uniform) this evaluation is redone or the host's
  const int label = blockIdx.x, tid = threadIdx.x;
  const int n_pred = t.n_pred;
  int n_gt = t.info[0], n_pairs = t.info[2];
  n_gt = n_gt < 0 ? 0 : (n_gt > t.gt_cap ? t.gt_cap : n_gt);
  n_pairs = n_pairs < 0 ? 0 : (n_pairs > t.pair_cap ? static_cast<int>(t.pair_cap) : n_pairs);
  if (tid < 2) cnt_s[tid] = 0;
  __syncthreads();
  int tp = 0, fp = 0;
  for (int p = tid; p < n_pred; p += kIeBlock) {
    if (!ie_kept(pr, p) || pr.label[p] != label || !(pr.conf[p] >= c.score_thr)) continue;
    int q0 = t.pred_pair_off[p], q1 = t.pred_pair_off[p + 1];
    if (q0 < 0) q0 = 0;
    if (q1 > n_pairs) q1 = n_pairs;
    double ov = 0.0;
    for (int q = q0; q < q1; ++q) {
      const double v = t.pb_iou[q];
      if (v > ov) ov = v;
    }
    if (ov >= c.iou_thr) ++tp;
    else ++fp;
  }
  if (tp) atomicAdd(&cnt_s[0], tp);
  if (fp) atomicAdd(&cnt_s[1], fp);
  double sum = 0.0, wsum = 0.0;                          // thread 0's
  int64_t vsum = 0, n = 0, hit = 0;
  for (int c0 = 0; c0 < n_gt; c0 += kIeBlock) {
    const int g = c0 + tid;
    const bool on = g < n_gt && t.gt_label[g] == label;
    double ov = 0.0;
    if (on) {
      int q0 = t.gt_pair_off[g], q1 = t.gt_pair_off[g + 1];
      if (q0 < 0) q0 = 0;
      if (q1 > n_pairs) q1 = n_pairs;
      for (int q = q0; q < q1; ++q) {
        const int p = t.pa_pred[q];
        if (p < 0 || p >= n_pred || !(pr.conf[p] >= c.score_thr)) continue;
        const double v = t.pa_iou[q];
        if (v > ov) ov = v;
      }
    }
    ov_s[tid] = ov;
    vert_s[tid] = on ? t.gt_vert[g] : 0;
    on_s[tid] = on ? 1 : 0;
    __syncthreads();
    if (tid == 0) {
      const int m = n_gt - c0 < kIeBlock ? n_gt - c0 : kIeBlock;
      for (int i = 0; i < m; ++i) {
        if (!on_s[i]) continue;
        sum = __dadd_rn(sum, ov_s[i]);
        wsum = __dadd_rn(wsum, __dmul_rn(ov_s[i], static_cast<double>(vert_s[i])));
        vsum += vert_s[i];
        ++n;
        hit += ov_s[i] >= c.iou_thr ? 1 : 0;
      }
    }
    __syncthreads();
  }
  __syncthreads();
  if (tid == 0) {
    // scans follow each other on the stream and a label is one workgroup's: plain updates
    const int L = c.n_labels;
    if (n > 0) {
      c.tallies[label] += 1;
      c.tallies[L + label] += n;
      c.tallies[2 * L + label] += hit;
      c.sums[label] = __dadd_rn(c.sums[label], __ddiv_rn(sum, static_cast<double>(n)));
      c.sums[L + label] = __dadd_rn(c.sums[L + label], __ddiv_rn(wsum, static_cast<double>(vsum)));
    }
    c.tallies[3 * L + label] += cnt_s[0];
    c.tallies[4 * L + label] += cnt_s[1];
  }
}

// ---- 4. curves (:146-199) -------------------------------------------------------------------------------
__global__ void __launch_bounds__(kIeBlock) ie_split_kernel(const uint64_t *__restrict__ key, int64_t n,
                                                            uint32_t *__restrict__ lo, int32_t *__restrict__ idx) {
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kIeBlock) + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kIeBlock) {
    lo[i] = static_cast<uint32_t>(key[i]);
    idx[i] = static_cast<int32_t>(i);
  }
}
// which: 0 high word of the key, 1 segment
__global__ void __launch_bounds__(kIeBlock) ie_gather_kernel(const uint64_t *__restrict__ key,
                                                             const uint32_t *__restrict__ meta, int which,
                                                             const int32_t *__restrict__ idx, int64_t n,
                                                             uint32_t *__restrict__ out) {
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kIeBlock) + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kIeBlock) {
    const int32_t j = idx[i];
    uint32_t v = 0;
    if (j >= 0 && j < n) v = which ? meta[j] >> 1 : static_cast<uint32_t>(key[j] >> 32);
    out[i] = v;
  }
}

__global__ void __launch_bounds__(kIeBlock) ie_seg_off_kernel(const int32_t *__restrict__ seg_stats, int n_seg,
                                                              int64_t *__restrict__ seg_off) {
  __shared__ int lds4[4];
  int64_t carry = 0;
  for (int c0 = 0; c0 < n_seg; c0 += kIeBlock) {
    const int s = c0 + threadIdx.x;
    const int cnt = s < n_seg ? seg_stats[s] : 0;
    int total = 0;
    const int incl = block_incl_scan_256(cnt, lds4, &total);
    if (s < n_seg) seg_off[s] = carry + incl - cnt;
    carry += total;
  }
}

// one workgroup per (label, threshold).  perm: the examples ordered by (segment, score).
__global__ void __launch_bounds__(kIeBlock) ie_curve_kernel(
    const uint64_t *__restrict__ ex_key, const uint32_t *__restrict__ ex_meta, const int32_t *__restrict__ perm,
    int64_t n_examples, const int32_t *__restrict__ seg_stats, const int64_t *__restrict__ seg_off, int n_seg,
    double *__restrict__ prec, double *__restrict__ rec, double *__restrict__ ap, double *__restrict__ rc,
    int32_t *__restrict__ flags) {
  __shared__ int lds4[4];
  __shared__ double red[kIeBlock];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int hard_fn = seg_stats[n_seg + s];
  const bool has_gt = seg_stats[2 * n_seg + s] != 0, has_pred = seg_stats[3 * n_seg + s] != 0;
  int64_t off = seg_off[s];
  int n = seg_stats[s];
  if (off < 0 || n < 0 || off + n > n_examples) n = 0, off = 0;     // (an overflowed accumulator; the caller redoes it)
  if (!(has_gt && has_pred) || n == 0) {
    if (tid == 0) {
      const double v = has_gt ? 0.0 : __longlong_as_double(0x7ff8000000000000LL);
      ap[s] = rc[s] = v;
      if (has_gt && has_pred) atomicOr(flags, SG_INST_NO_EXAMPLES);   // the reference's cum[-1] on an empty array
    }
    return;
  }
  double *P = prec + off + s, *R = rec + off + s;        // n + 1 entries each
  // y_true.sum()
  int n_true = 0;
  for (int c0 = 0; c0 < n; c0 += kIeBlock) {
    const int e = c0 + tid;
    int f = 0;
    if (e < n) {
      const int32_t j = perm[off + e];
      f = (j >= 0 && j < n_examples) ? static_cast<int>(ex_meta[j] & 1u) : 0;
    }
    int total = 0;
    block_incl_scan_256(f, lds4, &total);
    n_true += total;
  }
  // cumulative true count below each unique score (np.unique's first indices), precision and recall
  int carry_t = 0, carry_b = 0;
  for (int c0 = 0; c0 < n; c0 += kIeBlock) {
    const int e = c0 + tid;
    int f = 0, b = 0;
    if (e < n) {
      const int32_t j = perm[off + e];
      const bool ok = j >= 0 && j < n_examples;
      f = ok ? static_cast<int>(ex_meta[j] & 1u) : 0;
      const uint64_t k = ok ? ex_key[j] : 0;
      if (e == 0) {
        b = 1;
      } else {
        const int32_t jp = perm[off + e - 1];
        b = (jp >= 0 && jp < n_examples ? ex_key[jp] : 0) != k ? 1 : 0;
      }
    }
    int tot_t = 0, tot_b = 0;
    const int incl_t = block_incl_scan_256(f, lds4, &tot_t);
    const int incl_b = block_incl_scan_256(b, lds4, &tot_b);
    if (b) {
      const int i = carry_b + incl_b - 1;
      const int64_t below = carry_t + incl_t - f;
      const int64_t tp = n_true - below, fp = n - e - tp, fn = below + hard_fn;
      P[i] = static_cast<double>(tp) / static_cast<double>(tp + fp);
      R[i] = static_cast<double>(tp) / static_cast<double>(tp + fn);
    }
    carry_t += tot_t;
    carry_b += tot_b;
  }
  const int n_pr = carry_b + 1;
  if (tid == 0) {
    P[n_pr - 1] = 1.0;
    R[n_pr - 1] = 0.0;
  }
  __syncthreads();
  // np.dot(precision, np.convolve([r0, r..., 0], [-0.5, 0, 0.5], 'valid')), summed in a fixed order
  double acc = 0.0;
  for (int i = tid; i < n_pr; i += kIeBlock) {
    const double rl = R[i == 0 ? 0 : i - 1], rr = i + 1 < n_pr ? R[i + 1] : 0.0;
    acc += P[i] * (0.5 * rl + -0.5 * rr);
  }
  red[tid] = acc;
  __syncthreads();
  for (int w = kIeBlock / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    ap[s] = red[0];
    rc[s] = R[0];
  }
}

static int ie_seg_bits(int n_seg) {
  int b = 1;
  while ((1 << b) < n_seg) ++b;
  return b;
}

}  // namespace sg

using namespace sg;

extern "C" {

int64_t sg_inst_rle_run_slots(int64_t text_bytes, int n_masks) {
  if (text_bytes < 0 || n_masks < 0) return 0;
  return ie_slot_base(text_bytes, n_masks) + 1;
}

int sg_inst_rle_parse(const uint8_t *text, const int64_t *text_off, const int32_t *mask_pred, int n_masks,
                      int64_t text_bytes, int64_t length, int32_t *run_start, int32_t *run_len, int32_t *run_pred,
                      int64_t run_slots, int32_t *vert_count, int32_t *flags, sg_stream_t stream_) {
  SG_REQUIRE(n_masks >= 0 && text_bytes >= 0 && length >= 0 && length < (1LL << 31) && run_slots >= 0 && flags,
             "sg_inst_rle_parse: bad arguments");
  if (n_masks == 0) return SG_OK;
  SG_REQUIRE(text_off && run_start && run_len && run_pred && vert_count && (text_bytes == 0 || text),
             "sg_inst_rle_parse: null array");
  if (run_slots < sg_inst_rle_run_slots(text_bytes, n_masks)) {
    set_error("sg_inst_rle_parse: %lld run slots, %lld needed", static_cast<long long>(run_slots),
              static_cast<long long>(sg_inst_rle_run_slots(text_bytes, n_masks)));
    return SG_ERR_WORKSPACE;
  }
  ie_parse_kernel<<<n_masks, kIeBlock, 0, as_stream(stream_)>>>(text, text_off, mask_pred, text_bytes, length,
                                                               run_start, run_len, run_pred, run_slots, vert_count,
                                                               flags);
  return check_launch("sg_inst_rle_parse");
}

static bool ie_scan_args_ok(int64_t n_points, int n_pred, int64_t run_slots, int n_classes, int gt_cap, int n_thr,
                            int n_labels) {
  return n_points >= 0 && n_points < (1LL << 31) && n_pred >= 0 && run_slots >= 0 && run_slots < (1LL << 30) &&
         n_classes >= 1 && n_classes <= SG_EVAL_MAX_CLASSES && gt_cap >= 1 && gt_cap <= (1 << 20) && n_thr >= 1 &&
         n_thr <= SG_INST_MAX_THRESHOLDS && (n_labels == n_classes || n_labels == 1) &&
         static_cast<int64_t>(n_pred) * (gt_cap + 1) < (1LL << 28) &&
         static_cast<int64_t>(n_pred) * n_points < (1LL << 31);
}

size_t sg_inst_scan_workspace_bytes(int64_t n_points, int n_pred, int64_t run_slots, int n_classes, int gt_cap,
                                    int n_thr, int n_labels, int64_t *section_off) {
  if (!ie_scan_args_ok(n_points, n_pred, run_slots, n_classes, gt_cap, n_thr, n_labels)) return 0;
  IeScan t;
  size_t used = 0;
  ie_carve(nullptr, ~static_cast<size_t>(0) >> 1, n_pred, run_slots, n_classes, gt_cap, n_thr, n_labels, &t, &used,
           section_off);
  return used;
}

int sg_inst_scan_update(const int64_t *gts, int64_t n_points, const int32_t *run_start, const int32_t *run_len,
                        const int32_t *run_pred, int64_t run_slots, const int32_t *pred_label,
                        const int32_t *pred_vert, const double *pred_conf, int n_pred, int n_labels, int n_classes,
                        int64_t min_region, const double *thresholds, int n_thr, int gt_cap, uint64_t *ex_key,
                        uint32_t *ex_meta, int64_t ex_cap, int32_t *seg_stats, int64_t *totals, int32_t *flags,
                        void *ws, size_t ws_bytes, sg_stream_t stream_) {
  SG_REQUIRE(ie_scan_args_ok(n_points, n_pred, run_slots, n_classes, gt_cap, n_thr, n_labels) && thresholds &&
                 ex_cap >= 0 && seg_stats && totals && flags && ws && (ex_cap == 0 || (ex_key && ex_meta)) &&
                 (n_points == 0 || gts) && (n_pred == 0 || (pred_label && pred_vert && pred_conf)) &&
                 (run_slots == 0 || (run_start && run_len && run_pred)) && min_region >= 1,
             "sg_inst_scan_update: bad arguments");
  IeScan t;
  if (!ie_carve(ws, ws_bytes, n_pred, run_slots, n_classes, gt_cap, n_thr, n_labels, &t, nullptr, nullptr)) {
    set_error("sg_inst_scan_update: workspace too small");
    return SG_ERR_WORKSPACE;
  }
  hipStream_t stream = as_stream(stream_);
  hipMemsetAsync(ws, 0, t.zero_bytes, stream);
  if (n_points > 0)
    ie_gt_hist_kernel<<<grid_for(n_points, kIeBlock, 1024), kIeBlock, 0, stream>>>(gts, n_points, t.n_bins, t.hist,
                                                                                  flags);
  const int agnostic = n_labels == 1 && n_classes != 1;
  ie_gt_table_kernel<<<1, kIeBlock, 0, stream>>>(t, agnostic, flags);
  IePreds pr{pred_label, pred_vert, pred_conf, min_region};
  if (n_pred > 0 && run_slots > 0 && n_points > 0) {
    const int32_t *len = run_len;
    int32_t *off = t.run_off;
    const int64_t slots = run_slots;
    // run_off[r] = mask points before run r; [run_slots] = all of them (<= n_pred * n_points < 2**31)
    const int rc = exclusive_scan([len, slots] __device__(int64_t i) { return i < slots ? len[i] : 0; },
                                  [off] __device__(int64_t i, int v) { off[i] = v; }, run_slots + 1, nullptr,
                                  t.scan_ws, t.scan_ws_bytes, stream);
    if (rc != SG_OK) return rc;
    hipMemcpyAsync(t.info + 1, t.run_off + run_slots, 4, hipMemcpyDeviceToDevice, stream);
    ie_intersections_kernel<<<grid_for(static_cast<int64_t>(n_pred) * n_points, kIeBlock, 1024), kIeBlock, 0,
                              stream>>>(run_start, run_pred, gts, n_points, t);
  }
  ie_pairs_kernel<<<1, kIeBlock, 0, stream>>>(t, pr);
  IeThr thr;
  thr.n = n_thr;
  for (int i = 0; i < SG_INST_MAX_THRESHOLDS; ++i) thr.v[i] = i < n_thr ? thresholds[i] : 0.0;
  IeAcc acc{ex_key, ex_meta, ex_cap, seg_stats, totals, flags};
  ie_match_kernel<<<1, kIeBlock, 0, stream>>>(t, pr, thr, n_labels, acc);
  return check_launch("sg_inst_scan_update");
}

int sg_inst_scan_coverage(int64_t n_points, int n_pred, int64_t run_slots, int n_classes, int gt_cap, int n_thr,
                          int n_labels, const int32_t *pred_label, const int32_t *pred_vert,
                          const double *pred_conf, int64_t min_region, double iou_thr, double score_thr,
                          double *cov_sums, int64_t *tallies, const int32_t *flags, void *ws, size_t ws_bytes,
                          sg_stream_t stream_) {
  SG_REQUIRE(ie_scan_args_ok(n_points, n_pred, run_slots, n_classes, gt_cap, n_thr, n_labels) && cov_sums &&
                 tallies && flags && ws && (n_pred == 0 || (pred_label && pred_vert && pred_conf)) &&
                 min_region >= 1 && iou_thr == iou_thr && score_thr == score_thr,
             "sg_inst_scan_coverage: bad arguments");
  IeScan t;
  if (!ie_carve(ws, ws_bytes, n_pred, run_slots, n_classes, gt_cap, n_thr, n_labels, &t, nullptr, nullptr)) {
    set_error("sg_inst_scan_coverage: workspace too small");
    return SG_ERR_WORKSPACE;
  }
  IePreds pr{pred_label, pred_vert, pred_conf, min_region};
  IeCov c{iou_thr, score_thr, cov_sums, tallies, flags, n_labels};
  ie_coverage_kernel<<<n_labels, kIeBlock, 0, as_stream(stream_)>>>(t, pr, c);
  return check_launch("sg_inst_scan_coverage");
}

size_t sg_inst_curves_workspace_bytes(int64_t n_examples, int n_seg) {
  if (n_examples < 0 || n_seg < 1) return 0;
  const size_t n = static_cast<size_t>(n_examples);
  return 3 * align_up((n + 1) * 4) + 2 * align_up((n + n_seg + 1) * 8) + align_up(static_cast<size_t>(n_seg) * 8) +
         align_up(radix_sort_workspace_bytes(n_examples));
}

int sg_inst_curves(const uint64_t *ex_key, const uint32_t *ex_meta, int64_t n_examples, const int32_t *seg_stats,
                   int n_seg, double *ap, double *rc, int32_t *flags, void *ws, size_t ws_bytes,
                   sg_stream_t stream_) {
  SG_REQUIRE(n_examples >= 0 && n_examples < (1LL << 31) && n_seg >= 1 && n_seg <= (1 << 20) && seg_stats && ap &&
                 rc && flags && (n_examples == 0 || (ex_key && ex_meta)),
             "sg_inst_curves: bad arguments");
  if (ws_bytes < sg_inst_curves_workspace_bytes(n_examples, n_seg) || !ws) {
    set_error("sg_inst_curves: workspace too small");
    return SG_ERR_WORKSPACE;
  }
  hipStream_t stream = as_stream(stream_);
  Workspace w(ws, ws_bytes);
  const size_t n = static_cast<size_t>(n_examples);
  uint32_t *kbuf = w.take<uint32_t>(n + 1);
  uint32_t *kbuf2 = w.take<uint32_t>(n + 1);
  int32_t *idx = w.take<int32_t>(n + 1);
  double *prec = w.take<double>(n + n_seg + 1);
  double *rec = w.take<double>(n + n_seg + 1);
  int64_t *seg_off = w.take<int64_t>(n_seg);
  const size_t rs_bytes = radix_sort_workspace_bytes(n_examples);
  void *rs_ws = w.take<char>(rs_bytes);
  SG_REQUIRE(rs_ws, "sg_inst_curves: workspace too small");
  int32_t *perm = idx;
  if (n_examples > 0) {
    const int g = grid_for(n_examples, kIeBlock, 1024);
    uint32_t *ks;
    int32_t *vs;
    ie_split_kernel<<<g, kIeBlock, 0, stream>>>(ex_key, n_examples, kbuf, idx);
    int rc_ = radix_sort_pairs(kbuf, idx, n_examples, 32, rs_ws, rs_bytes, stream, &ks, &vs);
    if (rc_ != SG_OK) return rc_;
    ie_gather_kernel<<<g, kIeBlock, 0, stream>>>(ex_key, ex_meta, 0, vs, n_examples, kbuf2);
    if (vs != idx) hipMemcpyAsync(idx, vs, n * 4, hipMemcpyDeviceToDevice, stream);
    rc_ = radix_sort_pairs(kbuf2, idx, n_examples, 32, rs_ws, rs_bytes, stream, &ks, &vs);
    if (rc_ != SG_OK) return rc_;
    ie_gather_kernel<<<g, kIeBlock, 0, stream>>>(ex_key, ex_meta, 1, vs, n_examples, kbuf);
    if (vs != idx) hipMemcpyAsync(idx, vs, n * 4, hipMemcpyDeviceToDevice, stream);
    rc_ = radix_sort_pairs(kbuf, idx, n_examples, ie_seg_bits(n_seg), rs_ws, rs_bytes, stream, &ks, &vs);
    if (rc_ != SG_OK) return rc_;
    perm = vs;
  }
  ie_seg_off_kernel<<<1, kIeBlock, 0, stream>>>(seg_stats, n_seg, seg_off);
  ie_curve_kernel<<<n_seg, kIeBlock, 0, stream>>>(ex_key, ex_meta, perm, n_examples, seg_stats, seg_off, n_seg, prec,
                                                  rec, ap, rc, flags);
  return check_launch("sg_inst_curves");
}

}  // extern "C"
