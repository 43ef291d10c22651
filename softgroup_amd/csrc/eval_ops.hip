// eval_ops.hip -- the GPU half of instance evaluation: prediction x ground-truth
// intersection counts for ScanNetEval.assign_instances_for_scan
// (softgroup/evaluation/instance_eval.py:228-309), which the reference computes with one
// np.logical_and + count_nonzero over all N points per (prediction, GT instance) pair in a
// multiprocessing pool.  Here every mask point is visited once: masks arrive as runs (what the RLE
// strings hold), a thread per mask point looks up the point's GT slot and the wave adds one
// atomic per distinct (prediction, slot) it sees.
//   counts[p, slot]: slot < n_gt = GT instance index, slot == n_gt = "void" (label not evaluated)
// HBM-bound: total mask points * 4 B gathered + runs.
// Also the O(points) half of the point-wise and panoptic evaluators
// (softgroup/evaluation/point_wise_eval.py:4-44, panoptic_eval.py:24-166):
//   eval_tally_kernel: per-class seen / positive / correct over the valid points (gt != ignore) plus
//     the masked |offset_gt - offset_pred| sum, one pass; LDS histograms, one 64-bit atomic per
//     non-empty bin per workgroup; the fp64 offset partials go to a per-workgroup slab that one
//     workgroup reduces in fixed order (bitwise repeatable: the grid depends on N only).
//   pan_insert / pan_pairs / pan_unmatched: panoptic segments and (gt, pred) pairs counted in
//     open-addressing hash tables (CAS-inserted 64-bit keys), IoU per distinct pair, TP list, FP/FN.
#include "common.h"

namespace sg {

__global__ void __launch_bounds__(256) eval_intersections_kernel(const int32_t *__restrict__ run_start,
                                                                const int64_t *__restrict__ run_off,
                                                                const int32_t *__restrict__ run_pred,
                                                                int n_runs, int64_t total_points,
                                                                const int32_t *__restrict__ gt_slot,
                                                                int n_slots, int32_t *__restrict__ counts) {
  const int lane = threadIdx.x & 63;
  for (int64_t t0 = (blockIdx.x * 256LL + threadIdx.x) - lane; t0 < total_points; t0 += gridDim.x * 256LL) {
    const int64_t t = t0 + lane;
    const bool valid = t < total_points;
    int key = -1;
    if (valid) {
      int lo = 0, hi = n_runs;                 // last run with run_off[r] <= t
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (run_off[mid] <= t) lo = mid; else hi = mid;
      }
      const int point = run_start[lo] + static_cast<int>(t - run_off[lo]);
      key = run_pred[lo] * n_slots + gt_slot[point];
    }
    uint64_t todo = __ballot(valid);
    while (todo) {                             // one atomic per distinct (prediction, slot) of the wave
      const int leader = __ffsll(static_cast<long long>(todo)) - 1;
      const int k = __shfl(key, leader, 64);
      const uint64_t same = __ballot(valid && key == k) & todo;
      if (lane == leader) atomicAdd(&counts[k], __popcll(same));
      todo &= ~same;
    }
  }
}


// ---------------------------------------------------------------------------------------------
// point-wise / panoptic evaluation
// ---------------------------------------------------------------------------------------------
constexpr int kTallyBlock = 256;
constexpr int kTallyMaxGrid = 1024;
constexpr uint64_t kEvalEmpty = ~0ULL;

// element i of a label array of kind SG_EVAL_I32 / SG_EVAL_I64 / SG_EVAL_U32, widened to int64
__device__ __forceinline__ int64_t load_label(const void *p, int kind, int64_t i) {
  if (kind == SG_EVAL_I64) return static_cast<const int64_t *>(p)[i];
  const int32_t v = static_cast<const int32_t *>(p)[i];
  return kind == SG_EVAL_U32 ? static_cast<int64_t>(static_cast<uint32_t>(v)) : static_cast<int64_t>(v);
}

// elements i .. i+3 (i a multiple of 4; the caller's buffers are 16-byte aligned): 16-byte loads
// for a full group, scalar ones for the tail
__device__ __forceinline__ void load_label4(const void *p, int kind, int64_t i, int64_t n, int64_t v[4]) {
  if (i + 4 <= n) {
    if (kind == SG_EVAL_I64) {
      const longlong2 *q = reinterpret_cast<const longlong2 *>(static_cast<const int64_t *>(p) + i);
      const longlong2 a = q[0], b = q[1];
      v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    } else {
      const int4 a = *reinterpret_cast<const int4 *>(static_cast<const int32_t *>(p) + i);
      if (kind == SG_EVAL_U32) {
        v[0] = static_cast<uint32_t>(a.x); v[1] = static_cast<uint32_t>(a.y);
        v[2] = static_cast<uint32_t>(a.z); v[3] = static_cast<uint32_t>(a.w);
      } else {
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
      }
    }
  } else {
    for (int k = 0; k < 4; ++k) v[k] = i + k < n ? load_label(p, kind, i + k) : 0;
  }
}

// grid of the tally pass: a function of N only, so the fp64 partials are summed in the same order
// on every run and every device
static int tally_grid(int64_t n) { return grid_for((n + 3) / 4, kTallyBlock, kTallyMaxGrid); }

__global__ void __launch_bounds__(kTallyBlock) eval_tally_kernel(
    const void *__restrict__ pred, int pred_kind, const void *__restrict__ gt, int gt_kind, int64_t n,
    int64_t ignore, int panoptic, int n_classes, unsigned long long *__restrict__ tallies,
    const void *__restrict__ inst, int inst_kind, const float *__restrict__ off_pred,
    const float *__restrict__ off_gt, double *__restrict__ slab, unsigned long long *__restrict__ off_count,
    int32_t *__restrict__ flags) {
  __shared__ uint32_t h[3 * SG_EVAL_MAX_CLASSES];     // seen | positive | correct
  __shared__ double red[kTallyBlock];
  __shared__ uint32_t red_n[kTallyBlock];
  for (int c = threadIdx.x; c < 3 * n_classes; c += kTallyBlock) h[c] = 0;
  __syncthreads();
  uint32_t *seen = h, *positive = h + n_classes, *correct = h + 2 * n_classes;
  const bool with_cls = pred != nullptr, with_off = off_pred != nullptr;
  double acc = 0.0;
  uint32_t cnt = 0;
  int32_t bad = 0;
  for (int64_t i = (blockIdx.x * static_cast<int64_t>(kTallyBlock) + threadIdx.x) * 4; i < n;
       i += static_cast<int64_t>(gridDim.x) * kTallyBlock * 4) {
    int64_t p[4], g[4];
    if (with_cls) {
      load_label4(pred, pred_kind, i, n, p);
      load_label4(gt, gt_kind, i, n, g);
    }
    for (int k = 0; k < 4 && with_cls; ++k) {
      if (i + k >= n || g[k] == ignore) continue;
      int64_t pc = p[k];
      if (panoptic) {                     // x_sem = pred & 0xFFFF; ids must pack into 32 bits
        if (pc < 0 || pc > 0xFFFFFFFFLL) bad |= SG_EVAL_BAD_PRED;
        pc &= 0xFFFF;
      }
      const int64_t gc = g[k];
      if (gc < 0 || gc >= n_classes) {
        bad |= SG_EVAL_BAD_GT;            // the caller decides: an error (point-wise) or nowhere (panoptic)
      } else {
        atomicAdd(&seen[gc], 1u);
        if (pc == gc) atomicAdd(&correct[gc], 1u);
      }
      // predicted classes outside [0, n_classes) count nowhere (the fusion's ignore value among them)
      if (pc >= 0 && pc < n_classes) atomicAdd(&positive[pc], 1u);
    }
    if (with_off) {
      int64_t in[4];
      load_label4(inst, inst_kind, i, n, in);
      float a[12], b[12];
      if (i + 4 <= n) {
        const float4 *qa = reinterpret_cast<const float4 *>(off_gt + 3 * i);
        const float4 *qb = reinterpret_cast<const float4 *>(off_pred + 3 * i);
        for (int k = 0; k < 3; ++k) {
          const float4 x = qa[k], y = qb[k];
          a[4 * k] = x.x; a[4 * k + 1] = x.y; a[4 * k + 2] = x.z; a[4 * k + 3] = x.w;
          b[4 * k] = y.x; b[4 * k + 1] = y.y; b[4 * k + 2] = y.z; b[4 * k + 3] = y.w;
        }
      } else {
        for (int k = 0; k < 12; ++k) {
          a[k] = i * 3 + k < n * 3 ? off_gt[3 * i + k] : 0.f;
          b[k] = i * 3 + k < n * 3 ? off_pred[3 * i + k] : 0.f;
        }
      }
      // |gt - pred| is formed in float32 like numpy; only the sum is wider (fp64)
      for (int k = 0; k < 4; ++k) {
        if (i + k >= n || in[k] == ignore) continue;
        for (int d = 0; d < 3; ++d) acc += static_cast<double>(fabsf(a[3 * k + d] - b[3 * k + d]));
        ++cnt;
      }
    }
  }
  if (bad) atomicOr(flags, bad);
  __syncthreads();
  for (int c = threadIdx.x; c < 3 * n_classes; c += kTallyBlock)
    if (h[c]) atomicAdd(&tallies[c], static_cast<unsigned long long>(h[c]));
  if (with_off) {                         // fixed-order tree over the workgroup, one slab entry
    red[threadIdx.x] = acc;
    red_n[threadIdx.x] = cnt;
    __syncthreads();
    for (int s = kTallyBlock / 2; s > 0; s >>= 1) {
      if (threadIdx.x < s) {
        red[threadIdx.x] += red[threadIdx.x + s];
        red_n[threadIdx.x] += red_n[threadIdx.x + s];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      slab[blockIdx.x] = red[0];
      if (red_n[0]) atomicAdd(off_count, static_cast<unsigned long long>(red_n[0]));
    }
  }
}

// one workgroup: off_sum[0] += sum of slab[0 .. n_parts), in a fixed order
__global__ void __launch_bounds__(kTallyBlock) eval_slab_sum_kernel(const double *__restrict__ slab,
                                                                   int n_parts, double *__restrict__ off_sum) {
  __shared__ double red[kTallyBlock];
  double acc = 0.0;
  for (int j = threadIdx.x; j < n_parts; j += kTallyBlock) acc += slab[j];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = kTallyBlock / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) off_sum[0] += red[0];
}

// ---- panoptic: hash tables of segments and pairs -------------------------------------------
// pred segment key (scan << 48 | cl << 32 | x_inst), gt segment key (scan << 48 | cl << 32 | y_inst),
// pair key (pred slot << 32 | gt slot).  None can be all ones: cl < n_classes < 0xFFFF.
__device__ __forceinline__ uint32_t eval_hash_insert(uint64_t *keys, uint32_t mask, uint64_t key) {
  uint32_t s = static_cast<uint32_t>(mix64(key)) & mask;
  while (true) {
    const uint64_t seen = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (seen == key) return s;
    if (seen == kEvalEmpty) {
      const unsigned long long prev = atomicCAS(reinterpret_cast<unsigned long long *>(&keys[s]),
                                                static_cast<unsigned long long>(kEvalEmpty),
                                                static_cast<unsigned long long>(key));
      if (prev == kEvalEmpty || prev == key) return s;
    }
    s = (s + 1) & mask;
  }
}

// every lane of the wave calls this (ballots): one insert + one count atomic per distinct key of
// the wave (the points of a segment are mostly neighbours in a scan); returns the lane's slot
__device__ __forceinline__ uint32_t eval_insert_count(uint64_t *keys, uint32_t *cnt, uint32_t mask,
                                                      bool active, uint64_t key) {
  const int lane = threadIdx.x & 63;
  uint32_t mine = 0;
  uint64_t todo = __ballot(active);
  while (todo) {
    const int leader = __ffsll(static_cast<long long>(todo)) - 1;
    const uint64_t k = __shfl(key, leader, 64);
    const uint64_t same = __ballot(active && key == k) & todo;
    uint32_t s = 0;
    if (lane == leader) {
      s = eval_hash_insert(keys, mask, k);
      atomicAdd(&cnt[s], static_cast<uint32_t>(__popcll(same)));
    }
    s = __shfl(s, leader, 64);
    if ((same >> lane) & 1) mine = s;
    todo &= ~same;
  }
  return mine;
}

struct PanTables {
  uint64_t *pkey, *gkey, *qkey;           // pred segments, gt segments, pairs
  uint32_t *pcnt, *gcnt, *qcnt;
  uint8_t *pmatch, *gmatch;
  uint32_t cap;
};

static size_t pan_cap(int64_t n) {
  size_t c = 64;
  while (c < static_cast<size_t>(2 * n)) c <<= 1;     // load <= 1/2: every point a new key at worst
  return c;
}

static bool pan_carve(void *ws, size_t ws_bytes, int64_t n, PanTables *t) {
  Workspace w(ws, ws_bytes);
  const size_t cap = pan_cap(n);
  t->cap = static_cast<uint32_t>(cap);
  t->pkey = w.take<uint64_t>(cap);
  t->gkey = w.take<uint64_t>(cap);
  t->qkey = w.take<uint64_t>(cap);
  t->pcnt = w.take<uint32_t>(cap);
  t->gcnt = w.take<uint32_t>(cap);
  t->qcnt = w.take<uint32_t>(cap);
  t->pmatch = w.take<uint8_t>(cap);
  t->gmatch = w.take<uint8_t>(cap);
  return t->gmatch != nullptr;
}

__global__ void __launch_bounds__(256) pan_insert_kernel(
    const void *__restrict__ pred, int pred_kind, const void *__restrict__ sem, int sem_kind,
    const void *__restrict__ inst, int inst_kind, const int64_t *__restrict__ scan_off, int n_scans,
    int64_t n, int64_t ignore, int n_classes, PanTables t, int32_t *__restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const uint32_t mask = t.cap - 1;
  int32_t bad = 0;
  for (int64_t i0 = (blockIdx.x * 256LL + threadIdx.x) - lane; i0 < n; i0 += gridDim.x * 256LL) {
    const int64_t i = i0 + lane;
    bool is_p = false, is_g = false;
    uint64_t pk = 0, gk = 0;
    if (i < n) {
      const int64_t ys = load_label(sem, sem_kind, i);
      if (ys != ignore) {                 // only points outside the void area count
        int lo = 0, hi = n_scans;         // last scan with scan_off[s] <= i
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (scan_off[mid] <= i) lo = mid; else hi = mid;
        }
        const uint64_t scan = static_cast<uint64_t>(lo) << 48;
        const int64_t pv = load_label(pred, pred_kind, i);
        if (pv < 0 || pv > 0xFFFFFFFFLL) bad |= SG_EVAL_BAD_PRED;
        // x_sem = pred & 0xFFFF; x_inst = pred + 1, the WHOLE value with its class bits: all stuff
        // points of a class predicted with id 0 are one segment
        const int64_t xs = pv & 0xFFFF, x = pv + 1;
        if (xs < n_classes && pv >= 0) {
          is_p = true;
          pk = scan | static_cast<uint64_t>(xs) << 32 | static_cast<uint64_t>(x);
        }
        // y_inst: ignore -> -1, then + 2: ignored-instance gt points of a class are segment 1;
        // labels below -1 give y <= 0 and are no segment
        const int64_t iv = load_label(inst, inst_kind, i);
        const int64_t y = (iv == ignore ? -1 : iv) + 2;
        if (y >= (1LL << 31)) bad |= SG_EVAL_BAD_INST;
        if (ys >= 0 && ys < n_classes && y > 0 && y < (1LL << 31)) {
          is_g = true;
          gk = scan | static_cast<uint64_t>(ys) << 32 | static_cast<uint64_t>(y);
        }
      }
    }
    const uint32_t sp = eval_insert_count(t.pkey, t.pcnt, mask, is_p, pk);
    const uint32_t sg = eval_insert_count(t.gkey, t.gcnt, mask, is_g, gk);
    const bool is_q = is_p && is_g && ((pk >> 32) == (gk >> 32));     // same scan, same class
    eval_insert_count(t.qkey, t.qcnt, mask, is_q, static_cast<uint64_t>(sp) << 32 | sg);
  }
  if (bad) atomicOr(flags, bad);
}

// per distinct pair: U = area_gt + area_pred - I (int64), iou = I / U in double, TP when > 0.5
// (strictly).  IoU > 0.5 makes a segment's match unique, so the matched flags are race free.
__global__ void __launch_bounds__(256) pan_pairs_kernel(PanTables t, int64_t *__restrict__ tp_rows,
                                                        unsigned long long *__restrict__ tp_count) {
  for (int64_t s = blockIdx.x * 256LL + threadIdx.x; s < t.cap; s += gridDim.x * 256LL) {
    const uint64_t q = t.qkey[s];
    if (q == kEvalEmpty) continue;
    const uint32_t sp = static_cast<uint32_t>(q >> 32), sg = static_cast<uint32_t>(q);
    const int64_t inter = t.qcnt[s];
    const int64_t uni = static_cast<int64_t>(t.gcnt[sg]) + static_cast<int64_t>(t.pcnt[sp]) - inter;
    const double iou = static_cast<double>(inter) / static_cast<double>(uni);
    if (!(iou > 0.5)) continue;
    t.pmatch[sp] = 1;
    t.gmatch[sg] = 1;
    const uint64_t pk = t.pkey[sp], gk = t.gkey[sg];
    const unsigned long long r = atomicAdd(tp_count, 1ULL);
    int64_t *row = tp_rows + 4 * r;
    row[0] = static_cast<int64_t>(pk >> 32);                                  // scan << 16 | cl
    row[1] = static_cast<int64_t>((gk & 0xFFFFFFFFULL) << 32 | (pk & 0xFFFFFFFFULL));  // y * 2**32 + x
    row[2] = inter;
    row[3] = uni;
  }
}

// FP / FN per class: segments of at least min_points points that matched nothing (min_points
// never filters the IoU above)
__global__ void __launch_bounds__(256) pan_unmatched_kernel(PanTables t, int64_t min_points,
                                                            unsigned long long *__restrict__ fp,
                                                            unsigned long long *__restrict__ fn) {
  for (int64_t s = blockIdx.x * 256LL + threadIdx.x; s < t.cap; s += gridDim.x * 256LL) {
    const uint64_t pk = t.pkey[s], gk = t.gkey[s];
    if (pk != kEvalEmpty && static_cast<int64_t>(t.pcnt[s]) >= min_points && !t.pmatch[s])
      atomicAdd(&fp[(pk >> 32) & 0xFFFF], 1ULL);
    if (gk != kEvalEmpty && static_cast<int64_t>(t.gcnt[s]) >= min_points && !t.gmatch[s])
      atomicAdd(&fn[(gk >> 32) & 0xFFFF], 1ULL);
  }
}

static bool kind_ok(int k) { return k == SG_EVAL_I32 || k == SG_EVAL_I64 || k == SG_EVAL_U32; }

}  // namespace sg

using namespace sg;

extern "C" {

int sg_eval_intersections(const int32_t *run_start, const int64_t *run_off, const int32_t *run_pred,
                          int n_runs, int64_t total_points, const int32_t *gt_slot, int n_pred,
                          int n_slots, int32_t *counts, sg_stream_t stream_) {
  SG_REQUIRE(n_runs >= 0 && total_points >= 0 && n_pred >= 0 && n_slots >= 1,
             "sg_eval_intersections: bad arguments");
  hipStream_t stream = as_stream(stream_);
  hipMemsetAsync(counts, 0, static_cast<size_t>(n_pred) * n_slots * 4, stream);
  if (n_runs == 0 || total_points == 0) return check_launch("sg_eval_intersections");
  eval_intersections_kernel<<<grid_for(total_points, 256, 8192), 256, 0, stream>>>(
      run_start, run_off, run_pred, n_runs, total_points, gt_slot, n_slots, counts);
  return check_launch("sg_eval_intersections");
}

size_t sg_eval_tally_workspace_bytes(int64_t n_points) {
  return align_up(static_cast<size_t>(tally_grid(n_points < 0 ? 0 : n_points)) * sizeof(double));
}

int sg_eval_class_tally(const void *pred, int pred_kind, const void *gt, int gt_kind, int64_t n_points,
                        int64_t ignore_label, int panoptic, int n_classes, uint64_t *tallies,
                        const void *inst, int inst_kind, const float *offset_pred, const float *offset_gt,
                        double *offset_sum, uint64_t *offset_count, int32_t *flags, void *ws, size_t ws_bytes,
                        sg_stream_t stream_) {
  SG_REQUIRE(n_points >= 0 && n_classes >= 1 && n_classes <= SG_EVAL_MAX_CLASSES && kind_ok(pred_kind) &&
                 kind_ok(gt_kind) && flags && (!pred || (gt && tallies)),
             "sg_eval_class_tally: bad arguments");
  const bool with_off = offset_pred != nullptr;
  SG_REQUIRE(!with_off || (offset_gt && offset_sum && offset_count && kind_ok(inst_kind) &&
                           (n_points == 0 || inst)),
             "sg_eval_class_tally: offsets need offset_gt, inst, offset_sum and offset_count");
  SG_REQUIRE(!with_off || ws_bytes >= sg_eval_tally_workspace_bytes(n_points),
             "sg_eval_class_tally: workspace too small");
  if (n_points == 0) return SG_OK;
  hipStream_t stream = as_stream(stream_);
  const int grid = tally_grid(n_points);
  eval_tally_kernel<<<grid, kTallyBlock, 0, stream>>>(
      pred, pred_kind, gt, gt_kind, n_points, ignore_label, panoptic, n_classes,
      reinterpret_cast<unsigned long long *>(tallies), inst, inst_kind, offset_pred, offset_gt,
      static_cast<double *>(ws), reinterpret_cast<unsigned long long *>(offset_count), flags);
  if (with_off)
    eval_slab_sum_kernel<<<1, kTallyBlock, 0, stream>>>(static_cast<const double *>(ws), grid, offset_sum);
  return check_launch("sg_eval_class_tally");
}

size_t sg_eval_panoptic_workspace_bytes(int64_t n_points) {
  const size_t cap = pan_cap(n_points < 0 ? 0 : n_points);
  return 3 * align_up(cap * 8) + 3 * align_up(cap * 4) + 2 * align_up(cap);
}

int sg_eval_panoptic_segments(const void *pred, int pred_kind, const void *sem, int sem_kind,
                              const void *inst, int inst_kind, const int64_t *scan_off, int n_scans,
                              int64_t n_points, int64_t ignore_label, int n_classes, int64_t min_points,
                              uint64_t *fp_fn, int64_t *tp_rows, uint64_t *tp_count, int32_t *flags,
                              void *ws, size_t ws_bytes, sg_stream_t stream_) {
  SG_REQUIRE(n_points >= 0 && n_points < (1LL << 30) && n_scans >= 1 && n_scans <= 0xFFFF &&
                 n_classes >= 1 && n_classes < 0xFFFF && kind_ok(pred_kind) && kind_ok(sem_kind) &&
                 kind_ok(inst_kind) && fp_fn && tp_count && flags && (n_points == 0 || tp_rows) &&
                 (n_points == 0 || (pred && sem && inst && scan_off)),
             "sg_eval_panoptic_segments: bad arguments");
  PanTables t;
  SG_REQUIRE(pan_carve(ws, ws_bytes, n_points, &t), "sg_eval_panoptic_segments: workspace too small");
  if (n_points == 0) return hipMemsetAsync(tp_count, 0, 8, as_stream(stream_)) == hipSuccess ? SG_OK : SG_ERR_LAUNCH;
  hipStream_t stream = as_stream(stream_);
  const size_t cap = t.cap;
  hipMemsetAsync(tp_count, 0, 8, stream);
  hipMemsetAsync(t.pkey, 0xFF, cap * 8, stream);
  hipMemsetAsync(t.gkey, 0xFF, cap * 8, stream);
  hipMemsetAsync(t.qkey, 0xFF, cap * 8, stream);
  hipMemsetAsync(t.pcnt, 0, cap * 4, stream);
  hipMemsetAsync(t.gcnt, 0, cap * 4, stream);
  hipMemsetAsync(t.qcnt, 0, cap * 4, stream);
  hipMemsetAsync(t.pmatch, 0, cap, stream);
  hipMemsetAsync(t.gmatch, 0, cap, stream);
  pan_insert_kernel<<<grid_for(n_points, 256, 4096), 256, 0, stream>>>(
      pred, pred_kind, sem, sem_kind, inst, inst_kind, scan_off, n_scans, n_points, ignore_label, n_classes,
      t, flags);
  const int gc = grid_for(static_cast<int64_t>(cap), 256, 4096);
  pan_pairs_kernel<<<gc, 256, 0, stream>>>(t, tp_rows, reinterpret_cast<unsigned long long *>(tp_count));
  pan_unmatched_kernel<<<gc, 256, 0, stream>>>(t, min_points, reinterpret_cast<unsigned long long *>(fp_fn),
                                               reinterpret_cast<unsigned long long *>(fp_fn) + n_classes);
  return check_launch("sg_eval_panoptic_segments");
}

}  // extern "C"
