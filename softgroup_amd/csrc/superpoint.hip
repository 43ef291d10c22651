// superpoint.hip -- masks and labels snapped to an over-segmentation (sg_superpoint_index, sg_mask_snap,
// sg_superpoint_vote).
//
// The reference has no counterpart: it hands its masks and semantic labels out as the network left them.  Nearly
// every ScanNet / S3DIS pipeline refines both on "superpoints" (ScanNet ships `*.segs.json` with every scene): the
// points of one superpoint lie on one smooth patch, so a mask that covers most of a patch takes all of it and a mask
// that holds a few stray points of a patch gives them up.  This stage is new and opt-in; the rules are stated in
// include/softgroup_hip.h and softgroup_amd.ops.superpoint's numpy twins are the definition.
//
// index   validity + sort keys (a kernel of its own) -> stable radix sort of (id, point) -> head flags, one scan:
//         `order` (points segment after segment, ascending inside a segment), `seg_of`, `seg_start`, `meta`.
// snap    pass 1: a workgroup takes one TILE of kSpWalk consecutive positions of `order` and, one after another,
//         kSpMaskGroup masks; the tile's points and segments stay in registers, `inter` is counted per segment in
//         LDS.  A tile holds at most kSpWalk segments (each has a point).  A segment that lies inside the tile is
//         decided there; one that crosses a tile boundary adds its part to gcount[mask][tile of its first position]
//         (no two crossing segments begin in one tile) and is decided by the next launch.  Decisions are bits of the
//         `taken` matrix [n, ceil(S / 32)].
//         pass 2: a workgroup takes 2048 points and kSpMaskGroup masks; a wave turns 64 points into two words by
//         ballot, the populations go through LDS into npoint.
// vote    one wave per segment with a histogram in LDS; a segment longer than kSpWalk is walked in parts (its head
//         by its own wave, the rest by the waves of the tiles it covers) that add into ghist[tile of its first
//         position]; then the winner of the long ones, then one pass over the points.
//
// Integer adds and ORs only, one double division per decision; nothing that is written depends on the order of
// arrival.  Every loop is bounded by sizes the host passed; every index read from memory is range-checked before it
// addresses anything.
#include "common.h"
#include "radix_sort.h"
#include "scan.h"

namespace sg {

constexpr int kSpBlock = 256;
constexpr int kSpMaxInst = 16384;
constexpr int kSpWalk = SG_SUPERPOINT_WALK;               // positions of `order` per tile
constexpr int kSpItems = kSpWalk / kSpBlock;              // per thread
constexpr int kSpMaskGroup = 8;                           // masks per workgroup, one after another
constexpr int kSpMaxClasses = 256;
constexpr uint32_t kSpNoKey = 0x7FFFFFFFu;                // sort key of a point in no superpoint: behind every id
static_assert(kSpWalk % kSpBlock == 0 && kSpWalk % 64 == 0, "a tile is whole rounds of a workgroup");

inline int64_t sp_blocks(int64_t items, int per_block) { return items <= 0 ? 1 : (items + per_block - 1) / per_block; }

// ---- index -------------------------------------------------------------------------------------------------------
// One thread per point: the validity flag and the sort pair.  Nothing is indexed by an id, here or later.
__global__ void __launch_bounds__(kSpBlock) spi_keys_kernel(const int32_t *__restrict__ sp, int64_t n,
                                                           uint32_t *__restrict__ keys, int32_t *__restrict__ vals,
                                                           int32_t *__restrict__ meta) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kSpBlock) + threadIdx.x;
  if (i >= n) return;
  const int32_t v = sp[i];
  const bool bad = v < -1 || v == INT32_MAX;
  keys[i] = (v < 0 || bad) ? kSpNoKey : static_cast<uint32_t>(v);
  vals[i] = static_cast<int32_t>(i);
  if (bad) atomicOr(&meta[1], SG_SUPERPOINT_FLAG_ID);
}

struct SpiHeadIn {
  const uint32_t *key;
  const int32_t *flags;
  __device__ int operator()(int64_t j) const {
    if (*flags != 0) return 0;
    const uint32_t k = key[j];
    if (k == kSpNoKey) return 0;
    return (j == 0 || key[j - 1] != k) ? 1 : 0;
  }
};
struct SpiHeadOut {
  SpiHeadIn in;
  const int32_t *val;
  int64_t n;
  int32_t *order, *seg_of, *seg_start;
  __device__ void operator()(int64_t j, int before) const {      // before = heads in front of position j
    if (*in.flags != 0) return;
    const int32_t p = val[j];
    if (static_cast<uint32_t>(p) >= static_cast<uint64_t>(n)) return;        // (the sort moves pairs: never)
    if (in.key[j] == kSpNoKey) {
      seg_of[p] = -1;
      return;
    }
    const int h = in(j);
    const int64_t s = static_cast<int64_t>(before) + h - 1;
    if (s < 0 || s >= n) return;
    order[j] = p;
    seg_of[p] = static_cast<int32_t>(s);
    if (h) seg_start[s] = static_cast<int32_t>(j);
  }
};

// n_valid and the end of the last segment; meta[0] = S is the scan's total
__global__ void __launch_bounds__(kSpBlock) spi_tail_kernel(const uint32_t *__restrict__ key, int64_t n,
                                                           int32_t *__restrict__ seg_start, int32_t *__restrict__ meta) {
  if (meta[1] != 0) return;
  const int64_t j = blockIdx.x * static_cast<int64_t>(kSpBlock) + threadIdx.x;
  if (j >= n) return;
  const bool valid = key[j] != kSpNoKey;
  const bool next_valid = j + 1 < n && key[j + 1] != kSpNoKey;
  if (valid && !next_valid) {
    meta[2] = static_cast<int32_t>(j + 1);
    const int32_t S = meta[0];
    if (S >= 0 && S <= n) seg_start[S] = static_cast<int32_t>(j + 1);
  }
  if (j == 0 && !valid) seg_start[0] = 0;
}

__global__ void __launch_bounds__(kSpBlock) spi_largest_kernel(const int32_t *__restrict__ seg_start, int64_t n,
                                                              int32_t *__restrict__ meta) {
  if (meta[1] != 0) return;
  const int64_t s = blockIdx.x * static_cast<int64_t>(kSpBlock) + threadIdx.x;
  const int32_t S = meta[0];
  int size = 0;
  if (s < S && s < n) size = seg_start[s + 1] - seg_start[s];
  size = wave_max(size);
  if (lane_id() == 0 && size > 0) atomicMax(&meta[3], size);
}

static size_t spi_layout(int64_t n, void *base, uint32_t **keys, int32_t **vals, void **rs, size_t *rs_bytes, void **sc,
                         size_t *sc_bytes) {
  const size_t nn = static_cast<size_t>(n > 0 ? n : 1);
  const size_t rb = radix_sort_workspace_bytes(static_cast<int64_t>(nn)), sb = scan_workspace_bytes(static_cast<int64_t>(nn));
  size_t off = 0;
  char *b = static_cast<char *>(base);
  auto take = [&](size_t bytes) {
    char *r = b == nullptr ? nullptr : b + off;
    off += align_up(bytes);
    return r;
  };
  char *k = take(nn * 4), *v = take(nn * 4), *r = take(rb), *s = take(sb);
  if (base != nullptr) {
    *keys = reinterpret_cast<uint32_t *>(k), *vals = reinterpret_cast<int32_t *>(v);
    *rs = r, *rs_bytes = rb, *sc = s, *sc_bytes = sb;
  }
  return off + 256;
}

// ---- snap --------------------------------------------------------------------------------------------------------
struct SnapArgs {
  const uint32_t *bits;
  const int32_t *order, *seg_of, *seg_start;
  int n, mode;
  int32_t S;
  int64_t N, W, SW, n_valid, tiles, tile_stride;      // tiles = ceil(n_valid / kSpWalk) <= tile_stride
  double thr;
  uint32_t *taken;                 // [n, SW]
  int32_t *gcount;                 // [n, tile_stride]: inter of the crossing segment that begins in the tile
  uint32_t *out_bits;
  int32_t *npoint;
};

__device__ __forceinline__ bool snap_takes(int inter, int64_t size, double thr) {
  return inter >= 1 && static_cast<double>(inter) / static_cast<double>(size) > thr;
}

// grid (tiles, ceil(n / kSpMaskGroup))
__global__ void __launch_bounds__(kSpBlock) snap_count_kernel(SnapArgs a) {
  __shared__ int cnt[kSpWalk];
  const int tid = threadIdx.x;
  const int64_t lo = static_cast<int64_t>(blockIdx.x) * kSpWalk;
  const int64_t hi = lo + kSpWalk < a.n_valid ? lo + kSpWalk : a.n_valid;
  if (lo >= hi) return;
  // the tile's first segment (the same for every thread: the returns below are taken by all or by none)
  const int32_t p0 = a.order[lo];
  if (static_cast<uint32_t>(p0) >= static_cast<uint64_t>(a.N)) return;
  const int32_t s_first = a.seg_of[p0];
  if (s_first < 0 || s_first >= a.S) return;
  int32_t pp[kSpItems], sl[kSpItems], sa[kSpItems], sb[kSpItems];
#pragma unroll
  for (int r = 0; r < kSpItems; ++r) {
    const int64_t j = lo + r * kSpBlock + tid;
    pp[r] = -1, sl[r] = 0;
    if (j < hi) {
      const int32_t p = a.order[j];
      if (static_cast<uint32_t>(p) < static_cast<uint64_t>(a.N)) {
        const int32_t s = a.seg_of[p];
        const int64_t d = static_cast<int64_t>(s) - s_first;
        if (s >= 0 && s < a.S && d >= 0 && d < kSpWalk) pp[r] = p, sl[r] = static_cast<int32_t>(d);
      }
    }
    // local segment r * kSpBlock + tid of the tile: [sa, sb), sb = -1 when it is none of the tile's
    const int64_t s = static_cast<int64_t>(s_first) + r * kSpBlock + tid;
    sa[r] = 0, sb[r] = -1;
    if (s < a.S) {
      const int32_t b0 = a.seg_start[s], b1 = a.seg_start[s + 1];
      if (b0 >= 0 && b1 > b0 && b1 <= a.n_valid && b0 < hi && b1 > lo) sa[r] = b0, sb[r] = b1;
    }
  }
  for (int m = 0; m < kSpMaskGroup; ++m) {
    const int64_t k = static_cast<int64_t>(blockIdx.y) * kSpMaskGroup + m;
    if (k >= a.n) break;
#pragma unroll
    for (int r = 0; r < kSpItems; ++r) cnt[r * kSpBlock + tid] = 0;
    __syncthreads();
    const uint32_t *row = a.bits + k * a.W;
#pragma unroll
    for (int r = 0; r < kSpItems; ++r)
      if (pp[r] >= 0 && ((row[pp[r] >> 5] >> (pp[r] & 31)) & 1u)) atomicAdd(&cnt[sl[r]], 1);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kSpItems; ++r) {
      const int c = cnt[r * kSpBlock + tid];
      if (sb[r] < 0 || c <= 0) continue;
      if (sa[r] >= lo && sb[r] <= hi) {
        if (snap_takes(c, sb[r] - sa[r], a.thr)) {
          const int64_t s = static_cast<int64_t>(s_first) + r * kSpBlock + tid;
          atomicOr(&a.taken[k * a.SW + (s >> 5)], 1u << (s & 31));
        }
      } else {
        const int64_t t = sa[r] / kSpWalk;
        if (t < a.tiles) atomicAdd(&a.gcount[k * a.tile_stride + t], c);
      }
    }
    __syncthreads();
  }
}

// the segments that cross a tile boundary, by the tile they begin in; grid (ceil(tiles / block), n)
__global__ void __launch_bounds__(kSpBlock) snap_cross_kernel(SnapArgs a) {
  const int64_t t = blockIdx.x * static_cast<int64_t>(kSpBlock) + threadIdx.x;
  const int64_t k = blockIdx.y;
  if (t >= a.tiles || k >= a.n) return;
  const int64_t e = (t + 1) * kSpWalk - 1;                 // the tile's last position
  if (e + 1 >= a.n_valid) return;
  const int32_t p = a.order[e];
  if (static_cast<uint32_t>(p) >= static_cast<uint64_t>(a.N)) return;
  const int32_t s = a.seg_of[p];
  if (s < 0 || s >= a.S) return;
  const int32_t b0 = a.seg_start[s], b1 = a.seg_start[s + 1];
  if (b0 < 0 || b1 <= b0 || b1 > a.n_valid) return;
  if (b1 <= e + 1 || b0 / kSpWalk != t) return;            // ends with the tile / began in an earlier one
  if (snap_takes(a.gcount[k * a.tile_stride + t], b1 - b0, a.thr))
    atomicOr(&a.taken[k * a.SW + (s >> 5)], 1u << (s & 31));
}

// grid (ceil(N / kSpWalk), ceil(n / kSpMaskGroup))
__global__ void __launch_bounds__(kSpBlock) snap_apply_kernel(SnapArgs a) {
  __shared__ int acc[kSpMaskGroup];
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < kSpMaskGroup) acc[tid] = 0;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kSpWalk;
  int32_t sg[kSpItems];                                    // segment, -1 = none, -2 = beyond the cloud
#pragma unroll
  for (int r = 0; r < kSpItems; ++r) {
    const int64_t p = base + r * kSpBlock + tid;
    sg[r] = -2;
    if (p < a.N) {
      const int32_t s = a.seg_of[p];
      sg[r] = (s >= 0 && s < a.S) ? s : -1;
    }
  }
  __syncthreads();
  for (int m = 0; m < kSpMaskGroup; ++m) {
    const int64_t k = static_cast<int64_t>(blockIdx.y) * kSpMaskGroup + m;
    if (k >= a.n) break;
    const uint32_t *row = a.bits + k * a.W;
    const uint32_t *trow = a.taken + k * a.SW;
    uint32_t *orow = a.out_bits + k * a.W;
    int c = 0;
#pragma unroll
    for (int r = 0; r < kSpItems; ++r) {
      const int64_t p = base + r * kSpBlock + tid;
      bool out = false;
      if (sg[r] != -2) {
        const bool in = (row[p >> 5] >> (p & 31)) & 1u;
        if (sg[r] < 0) {
          out = in;
        } else {
          const bool tk = (trow[sg[r] >> 5] >> (sg[r] & 31)) & 1u;
          out = a.mode == SG_SNAP_SNAP ? tk : a.mode == SG_SNAP_GROW ? (in || tk) : (in && tk);
        }
      }
      const uint64_t bal = __ballot(out);
      if (lane == 0) {
        const int64_t w0 = (base + r * kSpBlock + (tid & ~63)) >> 5;
        if (w0 < a.W) orow[w0] = static_cast<uint32_t>(bal);
        if (w0 + 1 < a.W) orow[w0 + 1] = static_cast<uint32_t>(bal >> 32);
        c += __popcll(bal);
      }
    }
    if (lane == 0 && c) atomicAdd(&acc[m], c);
  }
  __syncthreads();
  if (tid < kSpMaskGroup) {
    const int64_t k = static_cast<int64_t>(blockIdx.y) * kSpMaskGroup + tid;
    if (k < a.n && acc[tid]) atomicAdd(&a.npoint[k], acc[tid]);
  }
}

static size_t snap_layout(int n, int64_t n_points, int64_t n_seg, void *base, uint32_t **taken, int32_t **gcount,
                          size_t *zero_bytes) {
  const size_t nn = static_cast<size_t>(n > 0 ? n : 1);
  const size_t sw = static_cast<size_t>((n_seg + 31) / 32), ts = static_cast<size_t>((n_points + kSpWalk - 1) / kSpWalk);
  const size_t tb = align_up(nn * (sw > 0 ? sw : 1) * 4), gb = align_up(nn * (ts > 0 ? ts : 1) * 4);
  if (base != nullptr) {
    *taken = reinterpret_cast<uint32_t *>(base);
    *gcount = reinterpret_cast<int32_t *>(static_cast<char *>(base) + tb);
    *zero_bytes = tb + gb;
  }
  return tb + gb + 256;
}

// ---- vote --------------------------------------------------------------------------------------------------------
struct VoteArgs {
  const int32_t *labels, *order, *seg_of, *seg_start;
  int64_t N, tiles;                // tiles = ceil(N / kSpWalk)
  int32_t S;
  int C, ignore;
  int32_t *seg_label;              // [S]
  int32_t *ghist;                  // [tiles, C]: histogram of the long segment that begins in the tile
  int32_t *out;
};

// [b0, b1) of segment s and the end of the last one; false when the index is not what the build wrote
__device__ __forceinline__ bool vote_segment(const VoteArgs &a, int64_t s, int64_t n_valid, int64_t *b0, int64_t *b1) {
  if (s < 0 || s >= a.S) return false;
  *b0 = a.seg_start[s], *b1 = a.seg_start[s + 1];
  return *b0 >= 0 && *b1 > *b0 && *b1 <= n_valid;
}

// the class with the greatest count, the lowest among equal counts, -1 when every count is 0; `mine(c)` = count of c
template <typename F>
__device__ __forceinline__ int vote_winner(int C, F mine) {
  int best = 0, cls = INT32_MAX;
  for (int c = lane_id(); c < C; c += 64) {
    const int v = mine(c);
    if (v > best) best = v, cls = c;                       // (ascending c: the first of equal counts stays)
  }
  const int top = wave_max(best);
  if (top <= 0) return -1;
  const int low = wave_max(best == top ? -cls : INT32_MIN);
  return -low;
}

// One wave per item: item s < S = segment s (all of it, or its head up to the next tile boundary when it is longer
// than a tile), item S + t = the part inside tile t of the long segment that covers the tile's first position.
__global__ void __launch_bounds__(kSpBlock) vote_count_kernel(VoteArgs a) {
  __shared__ int hist[kSpBlock / 64][kSpMaxClasses];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t item = blockIdx.x * static_cast<int64_t>(kSpBlock / 64) + wave;
  int64_t n_valid = a.seg_start[a.S];
  n_valid = n_valid < 0 ? 0 : n_valid > a.N ? a.N : n_valid;
  int64_t lo = 0, hi = 0, b0 = 0, b1 = 0, s = -1;
  bool whole = false;
  if (item < a.S) {
    s = item;
    if (vote_segment(a, s, n_valid, &b0, &b1)) {
      whole = b1 - b0 <= kSpWalk;
      const int64_t edge = (b0 / kSpWalk + 1) * kSpWalk;
      lo = b0, hi = whole || b1 < edge ? b1 : edge;
    }
  } else if (item - a.S < a.tiles) {
    const int64_t j0 = (item - a.S) * kSpWalk;
    if (j0 < n_valid) {
      const int32_t p = a.order[j0];
      if (static_cast<uint32_t>(p) < static_cast<uint64_t>(a.N)) {
        s = a.seg_of[p];
        if (vote_segment(a, s, n_valid, &b0, &b1) && b1 - b0 > kSpWalk && b0 < j0 && b1 > j0)
          lo = j0, hi = b1 < j0 + kSpWalk ? b1 : j0 + kSpWalk;
      }
    }
  }
  if (hi - lo > kSpWalk) hi = lo + kSpWalk;                // (never: a part is at most a tile)
  for (int c = lane; c < kSpMaxClasses; c += 64) hist[wave][c] = 0;
  __syncthreads();
  for (int64_t j = lo + lane; j < hi; j += 64) {
    const int32_t p = a.order[j];
    if (static_cast<uint32_t>(p) >= static_cast<uint64_t>(a.N)) continue;
    const int32_t l = a.labels[p];
    if (l >= 0 && l < a.C && l != a.ignore) atomicAdd(&hist[wave][l], 1);
  }
  __syncthreads();
  if (hi <= lo) return;                                    // (per wave; no barrier follows)
  if (whole) {
    const int *h = hist[wave];
    const int w = vote_winner(a.C, [h](int c) { return h[c]; });
    if (lane == 0) a.seg_label[s] = w;
  } else {
    const int64_t t = b0 / kSpWalk;
    if (t < a.tiles)
      for (int c = lane; c < a.C; c += 64)
        if (hist[wave][c]) atomicAdd(&a.ghist[t * a.C + c], hist[wave][c]);
  }
}

// One wave per tile: the winner of the long segment that begins in it (it covers the tile's last position).
__global__ void __launch_bounds__(kSpBlock) vote_long_kernel(VoteArgs a) {
  const int64_t t = blockIdx.x * static_cast<int64_t>(kSpBlock / 64) + (threadIdx.x >> 6);
  if (t >= a.tiles) return;
  int64_t n_valid = a.seg_start[a.S];
  n_valid = n_valid < 0 ? 0 : n_valid > a.N ? a.N : n_valid;
  const int64_t e = (t + 1) * kSpWalk - 1;
  if (e + 1 >= n_valid) return;
  const int32_t p = a.order[e];
  if (static_cast<uint32_t>(p) >= static_cast<uint64_t>(a.N)) return;
  const int64_t s = a.seg_of[p];
  int64_t b0, b1;
  if (!vote_segment(a, s, n_valid, &b0, &b1) || b1 - b0 <= kSpWalk || b0 / kSpWalk != t) return;
  const int32_t *g = a.ghist + t * a.C;
  const int w = vote_winner(a.C, [g](int c) { return g[c]; });
  if (lane_id() == 0) a.seg_label[s] = w;
}

__global__ void __launch_bounds__(kSpBlock) vote_apply_kernel(VoteArgs a) {
  const int64_t p = blockIdx.x * static_cast<int64_t>(kSpBlock) + threadIdx.x;
  if (p >= a.N) return;
  int32_t l = a.labels[p];
  const int32_t s = a.seg_of[p];
  if (s >= 0 && s < a.S) {
    const int32_t w = a.seg_label[s];
    if (w >= 0 && w < a.C) l = w;
  }
  a.out[p] = l;
}

static size_t vote_layout(int64_t n_points, int64_t n_seg, int n_classes, void *base, int32_t **ghist,
                          size_t *ghist_bytes, int32_t **seg_label) {
  const size_t ts = static_cast<size_t>((n_points + kSpWalk - 1) / kSpWalk);
  const size_t gb = align_up((ts > 0 ? ts : 1) * static_cast<size_t>(n_classes) * 4);
  const size_t lb = align_up(static_cast<size_t>(n_seg > 0 ? n_seg : 1) * 4);
  if (base != nullptr) {
    *ghist = reinterpret_cast<int32_t *>(base), *ghist_bytes = gb;
    *seg_label = reinterpret_cast<int32_t *>(static_cast<char *>(base) + gb);
  }
  return gb + lb + 256;
}

}  // namespace sg

using namespace sg;

extern "C" {

static bool sp_points_in_range(int64_t n_points) { return n_points >= 0 && n_points < (1LL << 31); }

size_t sg_superpoint_index_workspace_bytes(int64_t n_points) {
  if (!sp_points_in_range(n_points)) return 0;
  return spi_layout(n_points, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int sg_superpoint_index(const int32_t *sp, int64_t n_points, int32_t *order, int32_t *seg_of, int32_t *seg_start,
                        int32_t *meta, void *ws, size_t ws_bytes, sg_stream_t stream_) {
  if (!sp_points_in_range(n_points)) {
    set_error("sg_superpoint_index: n_points %lld outside the supported range (n_points < 2^31)",
              static_cast<long long>(n_points));
    return SG_ERR_UNSUPPORTED;
  }
  SG_REQUIRE(meta != nullptr && seg_start != nullptr, "sg_superpoint_index: null meta or seg_start");
  hipStream_t stream = as_stream(stream_);
  hipMemsetAsync(meta, 0, 4 * sizeof(int32_t), stream);
  if (n_points == 0) {
    hipMemsetAsync(seg_start, 0, sizeof(int32_t), stream);
    return check_launch("sg_superpoint_index");
  }
  SG_REQUIRE(sp != nullptr && order != nullptr && seg_of != nullptr, "sg_superpoint_index: null array");
  if (ws == nullptr || ws_bytes < sg_superpoint_index_workspace_bytes(n_points)) {
    set_error("sg_superpoint_index: workspace too small (%zu bytes, %zu needed)", ws_bytes,
              sg_superpoint_index_workspace_bytes(n_points));
    return SG_ERR_WORKSPACE;
  }
  uint32_t *keys;
  int32_t *vals;
  void *rs, *sc;
  size_t rs_bytes, sc_bytes;
  spi_layout(n_points, ws, &keys, &vals, &rs, &rs_bytes, &sc, &sc_bytes);
  const int grid = static_cast<int>(sp_blocks(n_points, kSpBlock));
  spi_keys_kernel<<<grid, kSpBlock, 0, stream>>>(sp, n_points, keys, vals, meta);
  uint32_t *ks;
  int32_t *vs;
  int rc = radix_sort_pairs(keys, vals, n_points, 31, rs, rs_bytes, stream, &ks, &vs);
  if (rc != SG_OK) return rc;
  const SpiHeadIn head{ks, meta + 1};
  rc = exclusive_scan(head, SpiHeadOut{head, vs, n_points, order, seg_of, seg_start}, n_points, meta, sc, sc_bytes,
                      stream);
  if (rc != SG_OK) return rc;
  spi_tail_kernel<<<grid, kSpBlock, 0, stream>>>(ks, n_points, seg_start, meta);
  spi_largest_kernel<<<grid, kSpBlock, 0, stream>>>(seg_start, n_points, meta);
  return check_launch("sg_superpoint_index");
}

static bool snap_in_range(int n_inst, int64_t n_points) {
  return n_inst >= 0 && n_inst <= kSpMaxInst && sp_points_in_range(n_points);
}

size_t sg_mask_snap_workspace_bytes(int n_inst, int64_t n_points, int64_t n_seg) {
  if (!snap_in_range(n_inst, n_points) || n_seg < 0 || n_seg > n_points) return 0;
  return snap_layout(n_inst, n_points, n_seg, nullptr, nullptr, nullptr, nullptr);
}

int sg_mask_snap(const uint32_t *bits, int n_inst, int64_t n_points, const int32_t *order, const int32_t *seg_of,
                 const int32_t *seg_start, int64_t n_seg, int64_t n_valid, double thr, int mode, uint32_t *out_bits,
                 int32_t *npoint, void *ws, size_t ws_bytes, sg_stream_t stream_) {
  if (!snap_in_range(n_inst, n_points)) {
    set_error("sg_mask_snap: n_inst %d, n_points %lld outside the supported range (n_inst <= %d, n_points < 2^31)",
              n_inst, static_cast<long long>(n_points), kSpMaxInst);
    return SG_ERR_UNSUPPORTED;
  }
  SG_REQUIRE(thr >= 0.0 && thr <= 1.0 && (mode == SG_SNAP_SNAP || mode == SG_SNAP_GROW || mode == SG_SNAP_TRIM),
             "sg_mask_snap: bad arguments (thr %g, mode %d)", thr, mode);
  SG_REQUIRE(n_seg >= 0 && n_seg <= n_valid && n_valid <= n_points && (n_seg == 0) == (n_valid == 0),
             "sg_mask_snap: %lld segments over %lld of %lld points", static_cast<long long>(n_seg),
             static_cast<long long>(n_valid), static_cast<long long>(n_points));
  if (n_inst == 0) return SG_OK;
  SG_REQUIRE(npoint != nullptr, "sg_mask_snap: null npoint");
  hipStream_t stream = as_stream(stream_);
  if (n_points == 0) {
    hipMemsetAsync(npoint, 0, static_cast<size_t>(n_inst) * 4, stream);
    return check_launch("sg_mask_snap");
  }
  SG_REQUIRE(bits != nullptr && out_bits != nullptr && seg_of != nullptr && bits != out_bits,
             "sg_mask_snap: null array, or out_bits is bits");
  SG_REQUIRE(n_seg == 0 || (order != nullptr && seg_start != nullptr), "sg_mask_snap: null index array");
  if (ws == nullptr || ws_bytes < sg_mask_snap_workspace_bytes(n_inst, n_points, n_seg)) {
    set_error("sg_mask_snap: workspace too small (%zu bytes, %zu needed)", ws_bytes,
              sg_mask_snap_workspace_bytes(n_inst, n_points, n_seg));
    return SG_ERR_WORKSPACE;
  }
  SnapArgs a;
  a.bits = bits, a.order = order, a.seg_of = seg_of, a.seg_start = seg_start;
  a.n = n_inst, a.mode = mode, a.S = static_cast<int32_t>(n_seg);
  a.N = n_points, a.W = (n_points + 31) / 32, a.SW = (n_seg + 31) / 32, a.n_valid = n_valid;
  a.tiles = (n_valid + kSpWalk - 1) / kSpWalk, a.tile_stride = (n_points + kSpWalk - 1) / kSpWalk;
  a.thr = thr, a.out_bits = out_bits, a.npoint = npoint;
  size_t zero_bytes;
  snap_layout(n_inst, n_points, n_seg, ws, &a.taken, &a.gcount, &zero_bytes);
  FillList f;
  f.add(a.taken, zero_bytes, 0);
  f.add(npoint, static_cast<size_t>(n_inst) * 4, 0);
  fill_many(f, stream);
  const unsigned groups = static_cast<unsigned>((n_inst + kSpMaskGroup - 1) / kSpMaskGroup);
  if (a.tiles > 0) {
    snap_count_kernel<<<dim3(static_cast<unsigned>(a.tiles), groups), kSpBlock, 0, stream>>>(a);
    if (a.tiles > 1)
      snap_cross_kernel<<<dim3(static_cast<unsigned>(sp_blocks(a.tiles, kSpBlock)), static_cast<unsigned>(n_inst)),
                          kSpBlock, 0, stream>>>(a);
  }
  snap_apply_kernel<<<dim3(static_cast<unsigned>(a.tile_stride), groups), kSpBlock, 0, stream>>>(a);
  return check_launch("sg_mask_snap");
}

size_t sg_superpoint_vote_workspace_bytes(int64_t n_points, int64_t n_seg, int n_classes) {
  if (!sp_points_in_range(n_points) || n_seg < 0 || n_seg > n_points || n_classes < 1 || n_classes > kSpMaxClasses)
    return 0;
  return vote_layout(n_points, n_seg, n_classes, nullptr, nullptr, nullptr, nullptr);
}

int sg_superpoint_vote(const int32_t *labels, int64_t n_points, const int32_t *order, const int32_t *seg_of,
                       const int32_t *seg_start, int64_t n_seg, int n_classes, int ignore_label, int32_t *out_labels,
                       int32_t *seg_label, void *ws, size_t ws_bytes, sg_stream_t stream_) {
  if (!sp_points_in_range(n_points) || n_classes < 1 || n_classes > kSpMaxClasses) {
    set_error("sg_superpoint_vote: n_points %lld, n_classes %d outside the supported range (n_points < 2^31, 1 <= "
              "n_classes <= %d)", static_cast<long long>(n_points), n_classes, kSpMaxClasses);
    return SG_ERR_UNSUPPORTED;
  }
  SG_REQUIRE(n_seg >= 0 && n_seg <= n_points, "sg_superpoint_vote: %lld segments over %lld points",
             static_cast<long long>(n_seg), static_cast<long long>(n_points));
  if (n_points == 0) return SG_OK;
  SG_REQUIRE(labels != nullptr && out_labels != nullptr && seg_of != nullptr && seg_start != nullptr &&
                 (n_seg == 0 || order != nullptr), "sg_superpoint_vote: null array");
  if (ws == nullptr || ws_bytes < sg_superpoint_vote_workspace_bytes(n_points, n_seg, n_classes)) {
    set_error("sg_superpoint_vote: workspace too small (%zu bytes, %zu needed)", ws_bytes,
              sg_superpoint_vote_workspace_bytes(n_points, n_seg, n_classes));
    return SG_ERR_WORKSPACE;
  }
  hipStream_t stream = as_stream(stream_);
  VoteArgs a;
  a.labels = labels, a.order = order, a.seg_of = seg_of, a.seg_start = seg_start;
  a.N = n_points, a.tiles = (n_points + kSpWalk - 1) / kSpWalk, a.S = static_cast<int32_t>(n_seg);
  a.C = n_classes, a.ignore = ignore_label, a.out = out_labels;
  size_t ghist_bytes;
  int32_t *own;
  vote_layout(n_points, n_seg, n_classes, ws, &a.ghist, &ghist_bytes, &own);
  a.seg_label = seg_label != nullptr ? seg_label : own;
  if (n_seg > 0) {
    constexpr int waves = kSpBlock / 64;
    hipMemsetAsync(a.ghist, 0, ghist_bytes, stream);
    vote_count_kernel<<<static_cast<unsigned>(sp_blocks(n_seg + a.tiles, waves)), kSpBlock, 0, stream>>>(a);
    vote_long_kernel<<<static_cast<unsigned>(sp_blocks(a.tiles, waves)), kSpBlock, 0, stream>>>(a);
  }
  vote_apply_kernel<<<static_cast<unsigned>(sp_blocks(n_points, kSpBlock)), kSpBlock, 0, stream>>>(a);
  return check_launch("sg_superpoint_vote");
}

}  // extern "C"
