// det_eval.hip -- axis-aligned 3D box detection AP (tools/eval_det.py of the reference) on gfx950.
//
// Box extraction (eval_det.py:280-313, coords[mask].min(0) / .max(0) per predicted mask and per GT
// instance): a thread per owned point, order-preserving uint64 keys of the float64 coordinates, a
// masked wave reduction per distinct owner of the wave and six 64-bit atomics per (wave, owner).
// Keys make min / max exact, so any visiting order gives the same bits.  The box buffer holds the keys
// while the points are reduced and is decoded in place at the end.
//
// Matching (eval_det_cls, eval_det.py:44-158): detection d's best GT -- (ovmax, jmax), the first GT
// of its (class, image) group with the strictly largest IoU -- depends on neither the order nor the
// threshold.  The greedy pass of the reference then makes d a TP exactly when ovmax > t and d is the
// earliest detection (in the host's sorted order) with that jmax and ovmax > t.  So: one thread per
// detection computes (ovmax, jmax) and claims its GT slot per threshold with an atomic min of its
// rank; a second pass flags the claim winners.  get_iou is restated operation for operation in fp64
// (built with -ffp-contract=off), including numpy's NaN-propagating minimum / maximum.
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr uint64_t kKeyMin0 = ~0ULL;      // identity of a min over keys
constexpr uint64_t kKeyMax0 = 0ULL;       // identity of a max over keys

// float64 -> uint64 key with the same order (negative: all bits flipped; non-negative: sign bit set)
__device__ __forceinline__ uint64_t dkey(double d) {
  const uint64_t u = static_cast<uint64_t>(__double_as_longlong(d));
  return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}
__device__ __forceinline__ double dkey_decode(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k ^ 0x8000000000000000ULL) : ~k;
  return __longlong_as_double(static_cast<long long>(u));
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

__device__ __forceinline__ double load_coord(const void *coords, int f64, int64_t i) {
  return f64 ? static_cast<const double *>(coords)[i] : static_cast<double>(static_cast<const float *>(coords)[i]);
}

// keys[6 o + a] = min key (a < 3) / max key (a >= 3)
__global__ void __launch_bounds__(kBlock) box_init_kernel(uint64_t *__restrict__ keys, int64_t n_owner,
                                                          unsigned long long *__restrict__ count,
                                                          unsigned long long *__restrict__ first) {
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kBlock) + threadIdx.x; i < n_owner * 6;
       i += static_cast<int64_t>(gridDim.x) * kBlock) {
    keys[i] = (i % 6) < 3 ? kKeyMin0 : kKeyMax0;
    if (count && i < n_owner) {
      count[i] = 0;
      first[i] = ~0ULL;
    }
  }
}

// Called by all 64 lanes of a wave (wave-uniform control flow).  Lanes with owner >= 0 contribute their
// point: per distinct owner of the wave one masked reduction and one set of atomics by the lowest lane
// holding it -- which, lanes visiting points in increasing order, also holds the owner's first point.
__device__ __forceinline__ void wave_commit(int64_t owner, const double x[3], int64_t point, uint64_t *keys,
                                            unsigned long long *count, unsigned long long *first) {
  const int lane = sg::lane_id();
  uint64_t todo = __ballot(owner >= 0);
  while (todo) {
    const int leader = __ffsll(static_cast<long long>(todo)) - 1;
    const int64_t k = __shfl(owner, leader, 64);
    const uint64_t same = __ballot(owner == k) & todo;
    const bool mine = (same >> lane) & 1;
    uint64_t lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const uint64_t key = dkey(x[a]);
      lo[a] = wave_min_u64(mine ? key : kKeyMin0);
      hi[a] = wave_max_u64(mine ? key : kKeyMax0);
    }
    if (lane == leader) {
      unsigned long long *b = reinterpret_cast<unsigned long long *>(keys + 6 * k);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        atomicMin(b + a, static_cast<unsigned long long>(lo[a]));
        atomicMax(b + 3 + a, static_cast<unsigned long long>(hi[a]));
      }
      if (count) {
        atomicAdd(count + k, static_cast<unsigned long long>(__popcll(same)));
        atomicMin(first + k, static_cast<unsigned long long>(point));
      }
    }
    todo &= ~same;
  }
}

// prediction masks as runs: run r covers points run_start[r] .. run_start[r] + len - 1 of owner
// run_owner[r]; run_off = exclusive prefix sum of the lengths.  A thread per mask point.
__global__ void __launch_bounds__(kBlock) box_runs_kernel(const void *__restrict__ coords, int f64,
                                                          const int64_t *__restrict__ run_start,
                                                          const int64_t *__restrict__ run_off,
                                                          const int32_t *__restrict__ run_owner, int64_t n_runs,
                                                          int64_t total, uint64_t *__restrict__ keys,
                                                          int32_t *__restrict__ flags) {
  const int lane = sg::lane_id();
  int32_t bad = 0;
  for (int64_t t0 = (blockIdx.x * static_cast<int64_t>(kBlock) + threadIdx.x) - lane; t0 < total;
       t0 += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t t = t0 + lane;
    int64_t owner = -1, p = 0;
    double x[3] = {0.0, 0.0, 0.0};
    if (t < total) {
      int64_t lo = 0, hi = n_runs;             // last run with run_off[r] <= t
      while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (run_off[mid] <= t) lo = mid; else hi = mid;
      }
      owner = run_owner[lo];
      p = run_start[lo] + (t - run_off[lo]);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        x[a] = load_coord(coords, f64, 3 * p + a);
        if (!isfinite(x[a])) bad = SG_DET_BAD_COORD;
      }
    }
    wave_commit(owner, x, p, keys, nullptr, nullptr);
  }
  if (bad) atomicOr(flags, bad);
}

// GT instance labels of n_scans scans laid end to end: point i of scan s (scan_off[s] <= i <
// scan_off[s+1]) with label l in [0, owner_off[s+1] - owner_off[s]) belongs to owner owner_off[s] + l.
__global__ void __launch_bounds__(kBlock) box_labels_kernel(const void *__restrict__ coords, int f64,
                                                            const int64_t *__restrict__ labels,
                                                            const int64_t *__restrict__ scan_off,
                                                            const int64_t *__restrict__ owner_off, int n_scans,
                                                            int64_t n_points, uint64_t *__restrict__ keys,
                                                            unsigned long long *__restrict__ count,
                                                            unsigned long long *__restrict__ first,
                                                            int32_t *__restrict__ flags) {
  const int lane = sg::lane_id();
  int32_t bad = 0;
  for (int64_t t0 = (blockIdx.x * static_cast<int64_t>(kBlock) + threadIdx.x) - lane; t0 < n_points;
       t0 += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t t = t0 + lane;
    int64_t owner = -1;
    double x[3] = {0.0, 0.0, 0.0};
    if (t < n_points) {
      int lo = 0, hi = n_scans;                // last scan with scan_off[s] <= t
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (scan_off[mid] <= t) lo = mid; else hi = mid;
      }
      const int64_t l = labels[t];
      if (l >= 0 && l < owner_off[lo + 1] - owner_off[lo]) {
        owner = owner_off[lo] + l;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          x[a] = load_coord(coords, f64, 3 * t + a);
          if (!isfinite(x[a])) bad = SG_DET_BAD_COORD;
        }
      }
    }
    wave_commit(owner, x, t, keys, count, first);
  }
  if (bad) atomicOr(flags, bad);
}

// keys -> float64 in place; owners without points get NaN, and first = -1
__global__ void __launch_bounds__(kBlock) box_decode_kernel(uint64_t *__restrict__ keys, int64_t n_owner,
                                                            const unsigned long long *__restrict__ count,
                                                            long long *__restrict__ first) {
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kBlock) + threadIdx.x; i < n_owner * 6;
       i += static_cast<int64_t>(gridDim.x) * kBlock) {
    const double v = dkey_decode(keys[i]);
    reinterpret_cast<double *>(keys)[i] = v;
    if (count && i < n_owner && count[i] == 0) first[i] = -1;
  }
}

// ---------------------------------------------------------------------------------------------
// matching
// ---------------------------------------------------------------------------------------------
struct Thresholds {
  double t[SG_DET_MAX_THRESHOLDS];
  int n;
};

// np.minimum / np.maximum: a NaN operand propagates
__device__ __forceinline__ double np_min(double a, double b) { return (a <= b || isnan(a)) ? a : b; }
__device__ __forceinline__ double np_max(double a, double b) { return (a >= b || isnan(a)) ? a : b; }

// get_iou (eval_det.py:44-66)
__device__ __forceinline__ double get_iou(const double *a, const double *b) {
  double min_max[3], max_min[3];
  bool all = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    min_max[k] = np_min(a[3 + k], b[3 + k]);
    max_min[k] = np_max(a[k], b[k]);
    all = all && (min_max[k] > max_min[k]);
  }
  if (!all) return 0.0;
  const double inter = ((min_max[0] - max_min[0]) * (min_max[1] - max_min[1])) * (min_max[2] - max_min[2]);
  const double vol_a = ((a[3] - a[0]) * (a[4] - a[1])) * (a[5] - a[2]);
  const double vol_b = ((b[3] - b[0]) * (b[4] - b[1])) * (b[5] - b[2]);
  const double uni = (vol_a + vol_b) - inter;
  return inter / uni;
}

// (ovmax, jmax) per detection (eval_det.py:120-135) and the claims: claim[thr * n_gt + jmax] = the
// lowest rank among detections with that jmax and ovmax > thr
__global__ void __launch_bounds__(kBlock) match_kernel(const double *__restrict__ det_box,
                                                       const int32_t *__restrict__ det_group,
                                                       const int32_t *__restrict__ det_rank, int64_t n_det,
                                                       const double *__restrict__ gt_box,
                                                       const int64_t *__restrict__ group_off, int64_t n_gt,
                                                       Thresholds th, double *__restrict__ ovmax_out,
                                                       int64_t *__restrict__ jmax_out, int32_t *__restrict__ claim) {
  for (int64_t d = blockIdx.x * static_cast<int64_t>(kBlock) + threadIdx.x; d < n_det;
       d += static_cast<int64_t>(gridDim.x) * kBlock) {
    double bb[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) bb[k] = det_box[6 * d + k];
    const int32_t g = det_group[d];
    double ovmax = -INFINITY;
    int64_t jmax = -1;
    for (int64_t j = group_off[g]; j < group_off[g + 1]; ++j) {
      double gb[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) gb[k] = gt_box[6 * j + k];
      const double iou = get_iou(bb, gb);
      if (iou > ovmax) {
        ovmax = iou;
        jmax = j;
      }
    }
    ovmax_out[d] = ovmax;
    jmax_out[d] = jmax;
    for (int k = 0; k < th.n; ++k)
      if (ovmax > th.t[k]) atomicMin(claim + k * n_gt + jmax, det_rank[d]);
  }
}

// tp[thr * n_det + d] = 1 when d won its claim (eval_det.py:137-146)
__global__ void __launch_bounds__(kBlock) flag_kernel(const int32_t *__restrict__ det_rank, int64_t n_det,
                                                      int64_t n_gt, Thresholds th, const double *__restrict__ ovmax,
                                                      const int64_t *__restrict__ jmax,
                                                      const int32_t *__restrict__ claim, uint8_t *__restrict__ tp) {
  for (int64_t d = blockIdx.x * static_cast<int64_t>(kBlock) + threadIdx.x; d < n_det;
       d += static_cast<int64_t>(gridDim.x) * kBlock) {
    const double o = ovmax[d];
    const int64_t j = jmax[d];
    for (int k = 0; k < th.n; ++k)
      tp[k * n_det + d] = (o > th.t[k] && claim[k * n_gt + j] == det_rank[d]) ? 1 : 0;
  }
}

}  // namespace

using namespace sg;

extern "C" {

int sg_det_boxes_runs(const void *coords, int coords_f64, const int64_t *run_start, const int64_t *run_off,
                      const int32_t *run_owner, int64_t n_runs, int64_t total_points, int64_t n_owner,
                      double *boxes, int32_t *flags, sg_stream_t stream_) {
  SG_REQUIRE(n_runs >= 0 && total_points >= 0 && n_owner >= 0 && flags && (n_owner == 0 || boxes) &&
                 (total_points == 0 || (coords && run_start && run_off && run_owner && n_runs > 0)),
             "sg_det_boxes_runs: bad arguments");
  if (n_owner == 0) return SG_OK;
  hipStream_t stream = as_stream(stream_);
  uint64_t *keys = reinterpret_cast<uint64_t *>(boxes);
  const int gi = grid_for(n_owner * 6, kBlock, 1024);
  box_init_kernel<<<gi, kBlock, 0, stream>>>(keys, n_owner, nullptr, nullptr);
  if (total_points > 0)
    box_runs_kernel<<<grid_for(total_points, kBlock, 8192), kBlock, 0, stream>>>(
        coords, coords_f64, run_start, run_off, run_owner, n_runs, total_points, keys, flags);
  box_decode_kernel<<<gi, kBlock, 0, stream>>>(keys, n_owner, nullptr, nullptr);
  return check_launch("sg_det_boxes_runs");
}

int sg_det_boxes_labels(const void *coords, int coords_f64, const int64_t *labels, const int64_t *scan_off,
                        const int64_t *owner_off, int n_scans, int64_t n_points, int64_t n_owner, double *boxes,
                        int64_t *count, int64_t *first, int32_t *flags, sg_stream_t stream_) {
  SG_REQUIRE(n_scans >= 1 && n_points >= 0 && n_owner >= 0 && flags &&
                 (n_owner == 0 || (boxes && count && first)) &&
                 (n_points == 0 || (coords && labels && scan_off && owner_off)),
             "sg_det_boxes_labels: bad arguments");
  if (n_owner == 0) return SG_OK;
  hipStream_t stream = as_stream(stream_);
  uint64_t *keys = reinterpret_cast<uint64_t *>(boxes);
  auto *cnt = reinterpret_cast<unsigned long long *>(count);
  auto *fst = reinterpret_cast<unsigned long long *>(first);
  const int gi = grid_for(n_owner * 6, kBlock, 1024);
  box_init_kernel<<<gi, kBlock, 0, stream>>>(keys, n_owner, cnt, fst);
  if (n_points > 0)
    box_labels_kernel<<<grid_for(n_points, kBlock, 8192), kBlock, 0, stream>>>(
        coords, coords_f64, labels, scan_off, owner_off, n_scans, n_points, keys, cnt, fst, flags);
  box_decode_kernel<<<gi, kBlock, 0, stream>>>(keys, n_owner, cnt, reinterpret_cast<long long *>(first));
  return check_launch("sg_det_boxes_labels");
}

size_t sg_det_match_workspace_bytes(int64_t n_gt, int n_thresholds) {
  return align_up(static_cast<size_t>(n_gt < 0 ? 0 : n_gt) * (n_thresholds < 0 ? 0 : n_thresholds) * 4);
}

int sg_det_match(const double *det_box, const int32_t *det_group, const int32_t *det_rank, int64_t n_det,
                 const double *gt_box, const int64_t *group_off, int64_t n_gt, const double *thresholds,
                 int n_thresholds, double *ovmax, int64_t *jmax, uint8_t *tp, void *ws, size_t ws_bytes,
                 sg_stream_t stream_) {
  SG_REQUIRE(n_det >= 0 && n_det < (1LL << 31) && n_gt >= 0 && n_thresholds >= 1 &&
                 n_thresholds <= SG_DET_MAX_THRESHOLDS && thresholds &&
                 (n_det == 0 || (det_box && det_group && det_rank && group_off && ovmax && jmax && tp)) &&
                 (n_gt == 0 || gt_box),
             "sg_det_match: bad arguments");
  SG_REQUIRE(ws_bytes >= sg_det_match_workspace_bytes(n_gt, n_thresholds) && (n_gt == 0 || ws),
             "sg_det_match: workspace too small");
  if (n_det == 0) return SG_OK;
  hipStream_t stream = as_stream(stream_);
  Thresholds th;
  th.n = n_thresholds;
  for (int k = 0; k < n_thresholds; ++k) th.t[k] = thresholds[k];
  int32_t *claim = static_cast<int32_t *>(ws);
  if (n_gt > 0) hipMemsetAsync(claim, 0x7F, static_cast<size_t>(n_gt) * n_thresholds * 4, stream);
  const int g = grid_for(n_det, kBlock, 4096);
  match_kernel<<<g, kBlock, 0, stream>>>(det_box, det_group, det_rank, n_det, gt_box, group_off, n_gt, th, ovmax,
                                         jmax, claim);
  flag_kernel<<<g, kBlock, 0, stream>>>(det_rank, n_det, n_gt, th, ovmax, jmax, claim, tp);
  return check_launch("sg_det_match");
}

}  // extern "C"
