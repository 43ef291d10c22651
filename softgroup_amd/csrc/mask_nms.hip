// mask_nms.hip -- greedy non-maximum suppression of instance masks held as bit rows (sg_mask_nms).
//
// The reference has no counterpart: its test path hands every (proposal, class) pair that passes the score and
// size cuts to the evaluators, which tolerate duplicates.  This stage is new, opt-in (test_cfg.nms) and runs on
// the rows sg_scan_instances leaves in the arena.  The rules are stated in include/softgroup_hip.h.
//
// Four launches and a fill, nothing synchronises, integer arithmetic only (the one division is IEEE double):
//   rows      one workgroup per row: population (bits at and beyond n_points masked off) and the extent of its
//             non-zero words.
//   rank      position of every mask in the visiting order: descending score, the LOWER index first among equal
//             scores (-0.0 == 0.0 by the float comparison).  One thread per mask against all the others.
//   pairs     one workgroup per pair of 4-row tiles (ti <= tj), lane = word: 8 coalesced loads and 16
//             popcount(a & b) accumulators per lane and step over the words where both tiles' extents overlap; the
//             waves split the word range and meet in LDS.  A pair over the threshold sets ONE bit of the decision
//             matrix, which is indexed by rank: row r holds the later masks the r-th mask in order would suppress
//             (integer atomicOr: the result does not depend on the order of arrival).  The n x n int32 matrix is
//             written only when the caller asks for it.
//   greedy    one wave walks the ranks 32 at a time: the 32 x 32 diagonal block decides who of the 32 survives
//             (readlane, no memory), then the survivors' rows are OR-ed into the `removed` vector in LDS with all
//             their loads independent -- two memory round trips per 32 masks, not one per mask.
#include "common.h"
#include "nms_greedy.h"

namespace sg {

constexpr int kNmsBlock = 256;
constexpr int kNmsTile = 4;
constexpr int kNmsMaxInst = 16384;
constexpr int kNmsMaxWords = kNmsMaxInst / 32;

__global__ void __launch_bounds__(kNmsBlock) nms_rows_kernel(const uint32_t *__restrict__ bits, int n, int64_t n_points,
                                                            int64_t words, int32_t *__restrict__ cnt,
                                                            int32_t *__restrict__ lo, int32_t *__restrict__ hi) {
  __shared__ int s_cnt[4], s_lo[4], s_hi[4];
  const int tid = threadIdx.x;
  const int tail = static_cast<int>(n_points & 31);
  for (int k = blockIdx.x; k < n; k += gridDim.x) {
    const uint32_t *row = bits + static_cast<int64_t>(k) * words;
    int c = 0;
    int64_t first = words, last = 0;
    for (int64_t w = tid; w < words; w += kNmsBlock) {
      uint32_t x = row[w];
      if (w == words - 1 && tail) x &= (1u << tail) - 1u;
      if (x) {
        c += __popc(x);
        first = w < first ? w : first;
        last = w + 1;
      }
    }
    int f = static_cast<int>(first), l = static_cast<int>(last);      // words <= 2^26
    c = wave_sum(c);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      f = min(f, __shfl_xor(f, o, 64));
      l = max(l, __shfl_xor(l, o, 64));
    }
    if ((tid & 63) == 0) s_cnt[tid >> 6] = c, s_lo[tid >> 6] = f, s_hi[tid >> 6] = l;
    __syncthreads();
    if (tid == 0) {
      cnt[k] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
      lo[k] = min(min(s_lo[0], s_lo[1]), min(s_lo[2], s_lo[3]));
      hi[k] = max(max(s_hi[0], s_hi[1]), max(s_hi[2], s_hi[3]));
    }
    __syncthreads();
  }
}

// rank[i] = masks visited before mask i; order[rank[i]] = i (the ranks are a permutation of 0 .. n-1)
__global__ void __launch_bounds__(kNmsBlock) nms_rank_kernel(const float *__restrict__ scores, int n,
                                                            int32_t *__restrict__ rank, int32_t *__restrict__ order) {
  for (int i = blockIdx.x * kNmsBlock + threadIdx.x; i < n; i += gridDim.x * kNmsBlock) {
    const float s = scores[i];
    int r = 0;
    for (int j = 0; j < n; ++j) {
      const float t = scores[j];
      r += (t > s || (t == s && j < i)) ? 1 : 0;
    }
    rank[i] = r;
    order[r] = i;
  }
}

struct NmsPairs {
  const uint32_t *bits;
  const int32_t *cnt, *lo, *hi, *rank, *labels;      // labels == nullptr: class-agnostic
  uint32_t *decide;                                  // [n, nw], by rank
  int32_t *inter_out;                                // [n, n] or nullptr
  double thr;
  int64_t n_points, words;
  int n, nw, measure;
};

__global__ void __launch_bounds__(kNmsBlock) nms_pairs_kernel(NmsPairs a) {
  __shared__ int part[4][kNmsTile * kNmsTile];
  const int tid = threadIdx.x, n = a.n;
  const int64_t nt = (n + kNmsTile - 1) / kNmsTile;
  const int tail = static_cast<int>(a.n_points & 31);
  for (int64_t p = blockIdx.x; p < nt * nt; p += gridDim.x) {
    const int ti = static_cast<int>(p / nt), tj = static_cast<int>(p - ti * nt);
    if (ti > tj) continue;                                      // (block-uniform, like every branch around a barrier here)
    int ra[kNmsTile], rb[kNmsTile];
    int a_lo = INT32_MAX, a_hi = 0, b_lo = INT32_MAX, b_hi = 0;
#pragma unroll
    for (int k = 0; k < kNmsTile; ++k) {
      ra[k] = min(ti * kNmsTile + k, n - 1);                    // (a ragged tile repeats its last row; not used below)
      rb[k] = min(tj * kNmsTile + k, n - 1);
      a_lo = min(a_lo, a.lo[ra[k]]), a_hi = max(a_hi, a.hi[ra[k]]);
      b_lo = min(b_lo, a.lo[rb[k]]), b_hi = max(b_hi, a.hi[rb[k]]);
    }
    const int64_t w_lo = max(a_lo, b_lo), w_hi = min(a_hi, b_hi);     // empty: every intersection is 0
    if (a.inter_out == nullptr) {
      if (w_lo >= w_hi) continue;
      if (a.labels != nullptr) {                                // class-aware: a tile pair without a common label
        bool common = false;
#pragma unroll
        for (int k = 0; k < kNmsTile; ++k)
#pragma unroll
          for (int l = 0; l < kNmsTile; ++l) common |= a.labels[ra[k]] == a.labels[rb[l]];
        if (!common) continue;
      }
    }
    int acc[kNmsTile * kNmsTile];
#pragma unroll
    for (int x = 0; x < kNmsTile * kNmsTile; ++x) acc[x] = 0;
    for (int64_t w = w_lo + tid; w < w_hi; w += kNmsBlock) {
      uint32_t va[kNmsTile], vb[kNmsTile];
#pragma unroll
      for (int k = 0; k < kNmsTile; ++k) {
        va[k] = a.bits[static_cast<int64_t>(ra[k]) * a.words + w];
        vb[k] = a.bits[static_cast<int64_t>(rb[k]) * a.words + w];
      }
      if (w == a.words - 1 && tail) {
#pragma unroll
        for (int k = 0; k < kNmsTile; ++k) va[k] &= (1u << tail) - 1u;
      }
#pragma unroll
      for (int k = 0; k < kNmsTile; ++k)
#pragma unroll
        for (int l = 0; l < kNmsTile; ++l) acc[k * kNmsTile + l] += __popc(va[k] & vb[l]);
    }
#pragma unroll
    for (int x = 0; x < kNmsTile * kNmsTile; ++x) {
      const int v = wave_sum(acc[x]);
      if ((tid & 63) == 0) part[tid >> 6][x] = v;
    }
    __syncthreads();
    if (tid < kNmsTile * kNmsTile) {
      const int k = tid / kNmsTile, l = tid % kNmsTile;
      const int i = ti * kNmsTile + k, j = tj * kNmsTile + l;
      if (i < n && j < n && (ti < tj || k <= l)) {
        const int inter = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
        if (a.inter_out != nullptr) {
          a.inter_out[static_cast<int64_t>(i) * n + j] = inter;
          a.inter_out[static_cast<int64_t>(j) * n + i] = inter;
        }
        if (i != j && (a.labels == nullptr || a.labels[i] == a.labels[j])) {
          const int64_t ci = a.cnt[i], cj = a.cnt[j];
          const int64_t den = a.measure == 0 ? ci + cj - inter : (ci < cj ? ci : cj);
          if (den > 0 && static_cast<double>(inter) / static_cast<double>(den) > a.thr) {
            const int ri = a.rank[i], rj = a.rank[j];
            const int first = min(ri, rj), later = max(ri, rj);
            atomicOr(&a.decide[static_cast<int64_t>(first) * a.nw + (later >> 5)], 1u << (later & 31));
          }
        }
      }
    }
    __syncthreads();
  }
}

// One wave.  removed: bit r = the mask of rank r is suppressed.
__global__ void __launch_bounds__(kWave) nms_greedy_kernel(const uint32_t *__restrict__ decide,
                                                          const int32_t *__restrict__ order, int n, int nw,
                                                          uint8_t *__restrict__ keep, int32_t *__restrict__ n_keep) {
  __shared__ uint32_t removed[kNmsMaxWords];
  const int lane = threadIdx.x;
  for (int w = lane; w < nw; w += kWave) removed[w] = 0;
  __syncthreads();
  int kept_total = 0;
  for (int c = 0; c < nw; ++c) {
    const int r = 32 * c + (lane & 31);
    uint32_t diag = 0;
    if (lane < 32 && r < n) diag = decide[static_cast<int64_t>(r) * nw + c];
    uint32_t cur = removed[c];
#pragma unroll
    for (int b = 0; b < 32; ++b) {
      const uint32_t row = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(diag), b));
      if (!((cur >> b) & 1u)) cur |= row;      // (row b only has bits above b: a later mask never suppresses an earlier one)
    }
    const int valid = n - 32 * c >= 32 ? 32 : n - 32 * c;
    const uint32_t kept = ~cur & (valid == 32 ? 0xFFFFFFFFu : (1u << valid) - 1u);
    kept_total += __popc(kept);
    if (lane < 32 && r < n) {
      const uint32_t o = static_cast<uint32_t>(order[r]);      // (a permutation for finite scores; a NaN must not write outside)
      if (o < static_cast<uint32_t>(n)) keep[o] = static_cast<uint8_t>((kept >> lane) & 1u);
    }
    for (int w = c + 1 + lane; w < nw; w += kWave) {
      uint32_t acc = removed[w];
      for (uint32_t m = kept; m; m &= m - 1) {
        const int b = __ffs(m) - 1;
        acc |= decide[static_cast<int64_t>(32 * c + b) * nw + w];
      }
      removed[w] = acc;
    }
    __syncthreads();
  }
  if (lane == 0) *n_keep = kept_total;
}

// nms_greedy.h: the same two kernels for the box NMS of box_ops.hip
void nms_rank_launch(const float *scores, int n, int32_t *rank, int32_t *order, hipStream_t stream) {
  nms_rank_kernel<<<grid_for(n, kNmsBlock, 1024), kNmsBlock, 0, stream>>>(scores, n, rank, order);
}

void nms_greedy_launch(const uint32_t *decide, const int32_t *order, int n, int nw, uint8_t *keep, int32_t *n_keep,
                       hipStream_t stream) {
  nms_greedy_kernel<<<1, kWave, 0, stream>>>(decide, order, n, nw, keep, n_keep);
}

}  // namespace sg

using namespace sg;

extern "C" {

static bool nms_in_range(int n_inst, int64_t n_points) {
  return n_inst >= 0 && n_inst <= kNmsMaxInst && n_points >= 0 && n_points < (1LL << 31);
}

size_t sg_mask_nms_workspace_bytes(int n_inst, int64_t n_points) {
  if (!nms_in_range(n_inst, n_points)) return 0;
  const size_t n = static_cast<size_t>(n_inst), nw = (n + 31) / 32;
  return 5 * align_up(n * 4 + 4) + align_up(n * nw * 4 + 4) + 256;
}

int sg_mask_nms(const uint32_t *bits, int n_inst, int64_t n_points, const float *scores, const int32_t *labels,
                double thr, int measure, int class_agnostic, uint8_t *keep, int32_t *n_keep, int32_t *inter_out,
                void *ws, size_t ws_bytes, sg_stream_t stream_) {
  if (!nms_in_range(n_inst, n_points)) {
    set_error("sg_mask_nms: n_inst %d, n_points %lld outside the supported range (n_inst <= %d, n_points < 2^31)",
              n_inst, static_cast<long long>(n_points), kNmsMaxInst);
    return SG_ERR_UNSUPPORTED;
  }
  SG_REQUIRE((measure == SG_NMS_IOU || measure == SG_NMS_MIN) && n_keep != nullptr && thr == thr,
             "sg_mask_nms: bad arguments (measure %d)", measure);
  SG_REQUIRE(n_inst == 0 || (scores != nullptr && keep != nullptr && (n_points == 0 || bits != nullptr)),
             "sg_mask_nms: null array");
  SG_REQUIRE(ws != nullptr && ws_bytes >= sg_mask_nms_workspace_bytes(n_inst, n_points),
             "sg_mask_nms: workspace too small");
  hipStream_t stream = as_stream(stream_);
  const int n = n_inst, nw = (n + 31) / 32;
  const int64_t words = (n_points + 31) / 32;
  Workspace w(ws, ws_bytes);
  int32_t *cnt = w.take<int32_t>(n + 1), *lo = w.take<int32_t>(n + 1), *hi = w.take<int32_t>(n + 1);
  int32_t *rank = w.take<int32_t>(n + 1), *order = w.take<int32_t>(n + 1);
  uint32_t *decide = w.take<uint32_t>(static_cast<size_t>(n) * nw + 1);
  SG_REQUIRE(decide != nullptr, "sg_mask_nms: workspace too small");
  if (n > 0) {
    FillList f;
    f.add(decide, static_cast<size_t>(n) * nw * 4, 0);
    fill_many(f, stream);
    nms_rows_kernel<<<grid_for(n, 1, 2048), kNmsBlock, 0, stream>>>(bits, n, n_points, words, cnt, lo, hi);
    nms_rank_kernel<<<grid_for(n, kNmsBlock, 1024), kNmsBlock, 0, stream>>>(scores, n, rank, order);
    NmsPairs a;
    a.bits = bits, a.cnt = cnt, a.lo = lo, a.hi = hi, a.rank = rank;
    a.labels = class_agnostic ? nullptr : labels;
    a.decide = decide, a.inter_out = inter_out, a.thr = thr;
    a.n_points = n_points, a.words = words, a.n = n, a.nw = nw, a.measure = measure;
    const int64_t nt = (n + kNmsTile - 1) / kNmsTile;
    nms_pairs_kernel<<<grid_for(nt * nt, 1, 1 << 16), kNmsBlock, 0, stream>>>(a);
  }
  nms_greedy_kernel<<<1, kWave, 0, stream>>>(decide, order, n, nw, keep, n_keep);
  return check_launch("sg_mask_nms");
}

}  // extern "C"
