// viz_io.hip -- colours and ASCII PLY text of a test run's point clouds, produced on the device.  Replaces the
// per-point work of the reference's tools/visualization.py: the instance paint (one full-array comparison per
// mask, :204-225 and :186-193), the class colour lookup through two dictionaries (:154-173) and write_ply's one
// str.format per vertex (:253-257).
//
// Streaming kernels, bytes-bound, in the shape of result_io.hip:
//   paint     masks come as bit rows (one word per 32 points) or as runs, which are first expanded to bit rows
//             (one lane per word: a binary search, then a walk over the runs that touch the word); a lane per
//             point then keeps the covering mask of the highest (priority, index).  pointnum = the mask's whole
//             population, whatever the paint leaves of it.
//   rank      stable ascending radix sort of (pointnum, index), read backwards: descending pointnum, the higher
//             index first among equals.
//   colours   table row per point -> uint8 RGB; the `input` task repeats the reference's float32 chain
//             ((c + 1) * 127.5) / 255 * 255 operation by operation (no contraction, IEEE divide) and truncates.
//   PLY       "%f %f %f %d %d %d\n" per kept point: line width -> exclusive scan -> bytes at the scanned offsets.
//             The floats are printed from integers: 24-bit mantissa * 10^6 (< 2^44), shifted by the exponent and
//             rounded half to even on the exact remainder -- what '%f' of the float32's exact value prints.
#include "common.h"
#include "radix_sort.h"
#include "scan.h"

namespace sg {

constexpr int kVizBlock = 256;
constexpr int kVizGtIds = 999;           // ids % 1000 - 1 lies in [-1, 998]
constexpr int32_t kVizNone = -100;       // label of a point no mask covers
static int viz_grid(int64_t items) { return grid_for(items, kVizBlock, 2048); }

// ---- masks ---------------------------------------------------------------------------------------------------
// bits[inst * words + w] from the runs of mask inst (ascending, disjoint, exclusive ends)
__global__ void __launch_bounds__(kVizBlock) viz_runs_to_bits_kernel(const int32_t *__restrict__ starts,
                                                                    const int32_t *__restrict__ ends,
                                                                    const int64_t *__restrict__ bounds, int64_t n_runs,
                                                                    int n_inst, int64_t n, int64_t words,
                                                                    uint32_t *__restrict__ bits) {
  const int64_t total = static_cast<int64_t>(n_inst) * words;
  for (int64_t g = blockIdx.x * static_cast<int64_t>(kVizBlock) + threadIdx.x; g < total;
       g += static_cast<int64_t>(gridDim.x) * kVizBlock) {
    const int64_t inst = g / words, base = (g - inst * words) * 32;
    const int64_t top = n - base < 32 ? n - base : 32;          // points of this word
    int64_t lo = bounds[inst], hi = bounds[inst + 1];
    lo = lo < 0 ? 0 : (lo > n_runs ? n_runs : lo);              // (a corrupt table must not leave the run arrays)
    hi = hi < lo ? lo : (hi > n_runs ? n_runs : hi);
    int64_t a = lo, b = hi;                                     // first run that ends behind `base`
    while (a < b) {
      const int64_t m = (a + b) >> 1;
      if (ends[m] > base) b = m; else a = m + 1;
    }
    uint32_t w = 0;
    for (int64_t r = a; r < hi; ++r) {
      int64_t s = static_cast<int64_t>(starts[r]) - base, e = static_cast<int64_t>(ends[r]) - base;
      if (s >= top) break;
      s = s < 0 ? 0 : s;
      e = e > top ? top : e;
      if (e > s) {
        const uint32_t upto_e = e >= 32 ? 0xFFFFFFFFu : (1u << e) - 1u;
        w |= upto_e & ~((1u << s) - 1u);
      }
    }
    bits[g] = w;
  }
}

// pointnum[k] = population of mask k (points below n only), 0 for a skipped mask.  One workgroup per mask.
__global__ void __launch_bounds__(kVizBlock) viz_pointnum_kernel(const uint32_t *__restrict__ bits, int64_t n,
                                                                int64_t words, const uint8_t *__restrict__ skip,
                                                                int32_t *__restrict__ pointnum) {
  __shared__ int lds4[4];
  const int k = blockIdx.x;
  int v = 0;
  if (skip == nullptr || skip[k] == 0) {
    const uint32_t *row = bits + static_cast<int64_t>(k) * words;
    const int tail = static_cast<int>(n & 31);
    for (int64_t w = threadIdx.x; w < words; w += kVizBlock) {
      uint32_t x = row[w];
      if (w == words - 1 && tail) x &= (1u << tail) - 1u;
      v += __popc(x);
    }
  }
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) pointnum[k] = lds4[0] + lds4[1] + lds4[2] + lds4[3];
}

// label[i] = the covering, non-skipped mask with the highest priority (the higher index among equals), or -100
__global__ void __launch_bounds__(kVizBlock) viz_paint_kernel(const uint32_t *__restrict__ bits, int n_inst, int64_t n,
                                                             int64_t words, const int32_t *__restrict__ priority,
                                                             const uint8_t *__restrict__ skip,
                                                             int32_t *__restrict__ label) {
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kVizBlock) + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kVizBlock) {
    const int64_t w = i >> 5;
    const int b = static_cast<int>(i & 31);
    int32_t best = kVizNone, best_p = 0;
    for (int k = 0; k < n_inst; ++k) {
      if (skip != nullptr && skip[k]) continue;
      if ((bits[static_cast<int64_t>(k) * words + w] >> b) & 1u) {
        const int32_t p = priority ? priority[k] : 0;
        if (best == kVizNone || p >= best_p) best = k, best_p = p;
      }
    }
    label[i] = best;
  }
}

// label = ids % 1000 - 1 (floor modulo, as numpy), counts[label] += 1 for label >= 0.  counts: kVizGtIds, zeroed.
__global__ void __launch_bounds__(kVizBlock) viz_gt_labels_kernel(const int64_t *__restrict__ ids, int64_t n,
                                                                 int32_t *__restrict__ label,
                                                                 int32_t *__restrict__ counts) {
  __shared__ int h[kVizGtIds];
  for (int j = threadIdx.x; j < kVizGtIds; j += kVizBlock) h[j] = 0;
  __syncthreads();
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kVizBlock) + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kVizBlock) {
    int64_t m = ids[i] % 1000;
    if (m < 0) m += 1000;
    const int32_t l = static_cast<int32_t>(m) - 1;
    label[i] = l;
    if (l >= 0) atomicAdd(&h[l], 1);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < kVizGtIds; j += kVizBlock)
    if (h[j]) atomicAdd(&counts[j], h[j]);
}

__global__ void __launch_bounds__(kVizBlock) viz_rank_keys_kernel(const int32_t *__restrict__ pointnum, int n_inst,
                                                                 uint32_t *__restrict__ keys, int32_t *__restrict__ vals) {
  const int k = blockIdx.x * kVizBlock + threadIdx.x;
  if (k < n_inst) {
    keys[k] = pointnum[k] < 0 ? 0u : static_cast<uint32_t>(pointnum[k]);
    vals[k] = k;
  }
}
// sorted ascending and stable; position j from the back is rank j
__global__ void __launch_bounds__(kVizBlock) viz_rank_fill_kernel(const int32_t *__restrict__ vals, int n_inst,
                                                                 int32_t *__restrict__ rank) {
  const int j = blockIdx.x * kVizBlock + threadIdx.x;
  if (j < n_inst) {
    const int32_t k = vals[j];
    if (k >= 0 && k < n_inst) rank[k] = n_inst - 1 - j;
  }
}

// ---- colours -------------------------------------------------------------------------------------------------
// meta[0] += labels outside the table, meta[1] += NaN colour components, meta[2] += components outside 0..255
__global__ void __launch_bounds__(kVizBlock) viz_colors_kernel(int mode, const float *__restrict__ colors,
                                                              const int64_t *__restrict__ cls,
                                                              const int32_t *__restrict__ inst,
                                                              const int32_t *__restrict__ rank, int n_rank,
                                                              const uint8_t *__restrict__ table, int k, int64_t n,
                                                              uint8_t *__restrict__ rgb, int64_t *__restrict__ meta) {
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kVizBlock) + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kVizBlock) {
    uint8_t out[3] = {0, 0, 0};
    if (mode == SG_VIZ_INPUT) {
      int nan = 0, wide = 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float r = __fmul_rn(__fadd_rn(colors[3 * i + c], 1.0f), 127.5f);
        const float v = __fmul_rn(__fdiv_rn(r, 255.0f), 255.0f);
        if (v != v) {
          ++nan;
        } else if (!(v > -1.0f && v < 256.0f)) {
          ++wide;
        } else {
          out[c] = static_cast<uint8_t>(static_cast<int>(v));       // (truncation; (-1, 0) -> 0)
        }
      }
      if (nan) atomicAdd(reinterpret_cast<unsigned long long *>(meta + 1), static_cast<unsigned long long>(nan));
      if (wide) atomicAdd(reinterpret_cast<unsigned long long *>(meta + 2), static_cast<unsigned long long>(wide));
    } else {
      int64_t row = -1;
      bool bad = false;
      if (mode == SG_VIZ_INSTANCE) {
        const int32_t l = inst[i];
        if (l >= n_rank)
          bad = true;
        else if (l >= 0)
          row = rank[l] % k;
      } else {
        int64_t l = cls[i];
        if (mode == SG_VIZ_CLASS_WRAP && l < 0) {
          l += k;                       // (numpy's negative index)
          bad = l < 0;
        }
        if (l >= k)
          bad = true;
        else if (l >= 0 && !bad)
          row = l;
      }
      if (bad) {
        atomicAdd(reinterpret_cast<unsigned long long *>(meta), 1ULL);
      } else if (row >= 0 && row < k) {
        out[0] = table[3 * row], out[1] = table[3 * row + 1], out[2] = table[3 * row + 2];
      }
    }
    rgb[3 * i] = out[0], rgb[3 * i + 1] = out[1], rgb[3 * i + 2] = out[2];
  }
}

// ---- PLY vertex lines ----------------------------------------------------------------------------------------
__device__ __forceinline__ int viz_digits32(uint32_t v) {
  return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5
       : v < 1000000u ? 6 : v < 10000000u ? 7 : v < 100000000u ? 8 : v < 1000000000u ? 9 : 10;
}

// x = (-1)^neg * q / 10^6 after rounding the exact value half to even at six decimals.  false: not finite or
// |x| >= 2^31 (the caller's numpy path prints those).
__device__ __forceinline__ bool viz_fixed6(float x, bool *neg, uint64_t *q_out) {
  const uint32_t b = __float_as_uint(x);
  const int e = static_cast<int>((b >> 23) & 0xFFu);
  const uint32_t m = b & 0x7FFFFFu;
  *neg = (b >> 31) != 0;
  if (e >= 158) return false;                                  // 2^31 and above, inf, nan
  const uint64_t p = static_cast<uint64_t>(e == 0 ? m : (m | 0x800000u)) * 1000000ULL;      // < 2^44
  const int s = e == 0 ? 149 : 150 - e;                        // x = mantissa * 2^-s
  uint64_t q;
  if (s <= 0) {
    q = p << (-s);                                             // (s >= -7: below 2^51)
  } else if (s >= 64) {
    q = 0;                                                     // p * 2^-64 < 2^-20: rounds to 0
  } else {
    q = p >> s;
    const uint64_t r = p & ((1ULL << s) - 1ULL), half = 1ULL << (s - 1);
    if (r > half || (r == half && (q & 1ULL))) ++q;
  }
  *q_out = q;
  return true;
}

struct VizVertexIn {
  const float *xyz, *offset;
  const uint8_t *rgb, *keep;
  __device__ __forceinline__ bool kept(int64_t i) const { return keep == nullptr || keep[i] != 0; }
  __device__ __forceinline__ float coord(int64_t i, int c) const {
    const float v = xyz[3 * i + c];
    return offset ? __fadd_rn(v, offset[3 * i + c]) : v;
  }
  // bytes of point i's line; 0 when it is not kept or declined
  __device__ __forceinline__ int width(int64_t i) const {
    if (!kept(i)) return 0;
    int w = 6;                                                 // five spaces and the newline
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      bool neg;
      uint64_t q;
      if (!viz_fixed6(coord(i, c), &neg, &q)) return 0;
      w += neg + viz_digits32(static_cast<uint32_t>(q / 1000000ULL)) + 7;
      const uint32_t v = rgb[3 * i + c];
      w += v < 10u ? 1 : v < 100u ? 2 : 3;
    }
    return w;
  }
};

// meta[0] = bytes of text, meta[1] += lines written, meta[2] += kept rows declined, meta[3] += lines that did not fit
__global__ void __launch_bounds__(kVizBlock) viz_ply_lines_kernel(VizVertexIn in, int64_t n,
                                                                 const int32_t *__restrict__ off,
                                                                 const int32_t *__restrict__ total, int64_t capacity,
                                                                 uint8_t *__restrict__ text, int64_t *__restrict__ meta) {
  if (blockIdx.x == 0 && threadIdx.x == 0) meta[0] = *total;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kVizBlock) + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kVizBlock) {
    if (!in.kept(i)) continue;
    bool neg[3], ok = true;
    uint64_t q[3];
    int w = 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      ok = viz_fixed6(in.coord(i, c), &neg[c], &q[c]) && ok;
      const uint32_t v = in.rgb[3 * i + c];
      w += v < 10u ? 1 : v < 100u ? 2 : 3;
    }
    if (!ok) {
      atomicAdd(reinterpret_cast<unsigned long long *>(meta + 2), 1ULL);
      continue;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) w += neg[c] + viz_digits32(static_cast<uint32_t>(q[c] / 1000000ULL)) + 7;
    const int64_t o = off[i];
    if (o + w > capacity) {
      atomicAdd(reinterpret_cast<unsigned long long *>(meta + 3), 1ULL);
      continue;
    }
    atomicAdd(reinterpret_cast<unsigned long long *>(meta + 1), 1ULL);
    uint8_t *p = text + o;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (neg[c]) *p++ = '-';
      uint32_t ip = static_cast<uint32_t>(q[c] / 1000000ULL);
      uint32_t fr = static_cast<uint32_t>(q[c] - static_cast<uint64_t>(ip) * 1000000ULL);
      const int d = viz_digits32(ip);
      for (int k = d - 1; k >= 0; --k) {
        p[k] = static_cast<uint8_t>('0' + ip % 10u);
        ip /= 10u;
      }
      p += d;
      *p++ = '.';
#pragma unroll
      for (int k = 5; k >= 0; --k) {
        p[k] = static_cast<uint8_t>('0' + fr % 10u);
        fr /= 10u;
      }
      p += 6;
      *p++ = ' ';
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint32_t v = in.rgb[3 * i + c];
      if (v >= 100u) *p++ = static_cast<uint8_t>('0' + v / 100u);
      if (v >= 10u) *p++ = static_cast<uint8_t>('0' + v / 10u % 10u);
      *p++ = static_cast<uint8_t>('0' + v % 10u);
      *p++ = c == 2 ? '\n' : ' ';
    }
  }
}

static int viz_paint_bits(const char *who, const uint32_t *bits, int n_inst, int64_t n, const int32_t *priority,
                          const uint8_t *skip, int32_t *label, int32_t *pointnum, hipStream_t stream) {
  const int64_t words = (n + 31) / 32;
  if (n_inst > 0) viz_pointnum_kernel<<<n_inst, kVizBlock, 0, stream>>>(bits, n, words, skip, pointnum);
  if (n > 0) viz_paint_kernel<<<viz_grid(n), kVizBlock, 0, stream>>>(bits, n_inst, n, words, priority, skip, label);
  return check_launch(who);
}

// the expansion sg_viz_paint_runs and sg_mask_bits_from_runs share
static void viz_runs_to_bits(const int32_t *starts, const int32_t *ends, const int64_t *bounds, int64_t n_runs,
                             int n_inst, int64_t n, uint32_t *bits, hipStream_t stream) {
  const int64_t words = (n + 31) / 32;
  const int64_t total = static_cast<int64_t>(n_inst) * words;
  if (total > 0)
    viz_runs_to_bits_kernel<<<viz_grid(total), kVizBlock, 0, stream>>>(starts, ends, bounds, n_runs, n_inst, n, words,
                                                                      bits);
}

}  // namespace sg

using namespace sg;

extern "C" {

constexpr int64_t kVizMaxPoints = (1LL << 31) - 64;
constexpr int64_t kVizMaxLines = (1LL << 31) / 72 - 1;      // 69 bytes per line at most: the offsets are int32

int sg_viz_paint_bits(const uint32_t *bits, int n_inst, int64_t n, const int32_t *priority, const uint8_t *skip,
                      int32_t *label, int32_t *pointnum, sg_stream_t stream) {
  SG_REQUIRE(n_inst >= 0 && n >= 0 && n <= kVizMaxPoints && (n == 0 || label != nullptr) &&
                 (n_inst == 0 || pointnum != nullptr) && (n_inst == 0 || n == 0 || bits != nullptr),
             "sg_viz_paint_bits: bad arguments (n_inst %d, n %lld)", n_inst, static_cast<long long>(n));
  return viz_paint_bits("sg_viz_paint_bits", bits, n_inst, n, priority, skip, label, pointnum, as_stream(stream));
}

size_t sg_viz_paint_runs_workspace_bytes(int n_inst, int64_t n) {
  const int64_t words = ((n > 0 ? n : 0) + 31) / 32;
  return align_up(static_cast<size_t>(n_inst > 0 ? n_inst : 0) * static_cast<size_t>(words) * 4) + 256;
}

int sg_viz_paint_runs(const int32_t *starts, const int32_t *ends, const int64_t *bounds, int64_t n_runs, int n_inst,
                      int64_t n, const int32_t *priority, const uint8_t *skip, int32_t *label, int32_t *pointnum,
                      void *ws, size_t ws_bytes, sg_stream_t stream_) {
  SG_REQUIRE(n_inst >= 0 && n >= 0 && n <= kVizMaxPoints && n_runs >= 0 && (n == 0 || label != nullptr) &&
                 (n_inst == 0 || (pointnum != nullptr && bounds != nullptr)) && (n_runs == 0 || (starts && ends)),
             "sg_viz_paint_runs: bad arguments (n_inst %d, n %lld)", n_inst, static_cast<long long>(n));
  SG_REQUIRE(ws != nullptr && ws_bytes >= sg_viz_paint_runs_workspace_bytes(n_inst, n),
             "sg_viz_paint_runs: workspace too small");
  hipStream_t stream = as_stream(stream_);
  uint32_t *bits = static_cast<uint32_t *>(ws);
  viz_runs_to_bits(starts, ends, bounds, n_runs, n_inst, n, bits, stream);
  return viz_paint_bits("sg_viz_paint_runs", bits, n_inst, n, priority, skip, label, pointnum, stream);
}

int sg_mask_bits_from_runs(const int32_t *starts, const int32_t *ends, const int64_t *bounds, int64_t n_runs,
                           int n_inst, int64_t n, uint32_t *bits, sg_stream_t stream) {
  SG_REQUIRE(n_inst >= 0 && n >= 0 && n <= kVizMaxPoints && n_runs >= 0 && (n_inst == 0 || bounds != nullptr) &&
                 (n_runs == 0 || (starts && ends)) && (n_inst == 0 || n == 0 || bits != nullptr),
             "sg_mask_bits_from_runs: bad arguments (n_inst %d, n %lld)", n_inst, static_cast<long long>(n));
  viz_runs_to_bits(starts, ends, bounds, n_runs, n_inst, n, bits, as_stream(stream));
  return check_launch("sg_mask_bits_from_runs");
}

int sg_viz_gt_labels(const int64_t *ids, int64_t n, int32_t *label, int32_t *pointnum, sg_stream_t stream_) {
  SG_REQUIRE(n >= 0 && n <= kVizMaxPoints && pointnum != nullptr && (n == 0 || (ids && label)),
             "sg_viz_gt_labels: bad arguments (n %lld)", static_cast<long long>(n));
  hipStream_t stream = as_stream(stream_);
  hipMemsetAsync(pointnum, 0, kVizGtIds * sizeof(int32_t), stream);
  if (n > 0) viz_gt_labels_kernel<<<grid_for(n, kVizBlock, 256), kVizBlock, 0, stream>>>(ids, n, label, pointnum);
  return check_launch("sg_viz_gt_labels");
}

size_t sg_viz_instance_rank_workspace_bytes(int n_inst) {
  const int64_t m = n_inst > 0 ? n_inst : 1;
  return 2 * align_up(static_cast<size_t>(m) * 4) + align_up(radix_sort_workspace_bytes(m)) + 256;
}

int sg_viz_instance_rank(const int32_t *pointnum, int n_inst, int32_t *rank, void *ws, size_t ws_bytes,
                         sg_stream_t stream_) {
  SG_REQUIRE(n_inst >= 0 && (n_inst == 0 || (pointnum && rank)), "sg_viz_instance_rank: bad arguments (n_inst %d)",
             n_inst);
  SG_REQUIRE(ws != nullptr && ws_bytes >= sg_viz_instance_rank_workspace_bytes(n_inst),
             "sg_viz_instance_rank: workspace too small");
  if (n_inst == 0) return SG_OK;
  hipStream_t stream = as_stream(stream_);
  Workspace a(ws, ws_bytes);
  uint32_t *keys = a.take<uint32_t>(n_inst);
  int32_t *vals = a.take<int32_t>(n_inst);
  const size_t sbytes = radix_sort_workspace_bytes(n_inst);
  void *sws = a.take<char>(sbytes);
  const int grid = (n_inst + kVizBlock - 1) / kVizBlock;
  viz_rank_keys_kernel<<<grid, kVizBlock, 0, stream>>>(pointnum, n_inst, keys, vals);
  uint32_t *ks = nullptr;
  int32_t *vs = nullptr;
  const int rc = radix_sort_pairs(keys, vals, n_inst, 32, sws, sbytes, stream, &ks, &vs);
  if (rc != SG_OK) return rc;
  viz_rank_fill_kernel<<<grid, kVizBlock, 0, stream>>>(vs, n_inst, rank);
  return check_launch("sg_viz_instance_rank");
}

int sg_viz_colors(int mode, const float *colors, const int64_t *cls, const int32_t *inst, const int32_t *rank,
                  int n_rank, const uint8_t *table, int k, int64_t n, uint8_t *rgb, int64_t *meta,
                  sg_stream_t stream_) {
  SG_REQUIRE(n >= 0 && n <= kVizMaxPoints && meta != nullptr && (n == 0 || rgb != nullptr),
             "sg_viz_colors: bad arguments (n %lld)", static_cast<long long>(n));
  SG_REQUIRE(mode == SG_VIZ_INPUT || mode == SG_VIZ_CLASS || mode == SG_VIZ_CLASS_WRAP || mode == SG_VIZ_INSTANCE,
             "sg_viz_colors: unknown mode %d", mode);
  if (mode == SG_VIZ_INPUT) {
    SG_REQUIRE(n == 0 || colors != nullptr, "sg_viz_colors: the input task needs colors");
  } else {
    SG_REQUIRE(table != nullptr && k > 0, "sg_viz_colors: a colour table is needed");
    SG_REQUIRE(n == 0 || (mode == SG_VIZ_INSTANCE ? (inst != nullptr && n_rank >= 0 && (n_rank == 0 || rank != nullptr))
                                                  : cls != nullptr),
               "sg_viz_colors: labels missing");
  }
  hipStream_t stream = as_stream(stream_);
  hipMemsetAsync(meta, 0, 3 * sizeof(int64_t), stream);
  if (n > 0)
    viz_colors_kernel<<<viz_grid(n), kVizBlock, 0, stream>>>(mode, colors, cls, inst, rank, n_rank, table, k, n, rgb,
                                                            meta);
  return check_launch("sg_viz_colors");
}

size_t sg_viz_ply_vertices_workspace_bytes(int64_t n) {
  const int64_t m = n > 0 ? n : 1;
  return align_up(static_cast<size_t>(m) * 4) + align_up(scan_workspace_bytes(m)) + 512;
}

int sg_viz_ply_vertices(const float *xyz, const float *offset, const uint8_t *rgb, const uint8_t *keep, int64_t n,
                        uint8_t *text, int64_t text_capacity, int64_t *meta, void *ws, size_t ws_bytes,
                        sg_stream_t stream_) {
  SG_REQUIRE(n >= 0 && n <= kVizMaxLines && meta != nullptr && text_capacity >= 0 && (n == 0 || (xyz && rgb && text)),
             "sg_viz_ply_vertices: bad arguments (n %lld)", static_cast<long long>(n));
  SG_REQUIRE(ws != nullptr && ws_bytes >= sg_viz_ply_vertices_workspace_bytes(n),
             "sg_viz_ply_vertices: workspace too small");
  hipStream_t stream = as_stream(stream_);
  hipMemsetAsync(meta, 0, 4 * sizeof(int64_t), stream);
  if (n == 0) return check_launch("sg_viz_ply_vertices");
  Workspace a(ws, ws_bytes);
  int32_t *off = a.take<int32_t>(n);
  const size_t sbytes = scan_workspace_bytes(n);
  void *sws = a.take<char>(sbytes);
  int32_t *total = a.take<int32_t>(64);
  const VizVertexIn in{xyz, offset, rgb, keep};
  const int rc = exclusive_scan([in] __device__(int64_t i) { return in.width(i); },
                                [off] __device__(int64_t i, int v) { off[i] = v; }, n, total, sws, sbytes, stream);
  if (rc != SG_OK) return rc;
  viz_ply_lines_kernel<<<viz_grid(n), kVizBlock, 0, stream>>>(in, n, off, total, text_capacity, text, meta);
  return check_launch("sg_viz_ply_vertices");
}

}  // extern "C"
