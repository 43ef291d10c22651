// stitch.hip -- large clouds cut into overlapping tiles, every tile scanned at full resolution, and the instances
// that straddle a cut joined again: tile membership (sg_tile_assign_count / _fill), the points two tiles share
// (sg_tile_shared), rectangular mask intersections and the link decision (sg_mask_cross_links), connected
// components of the link graph (sg_stitch_components), global ids of the set bits of tile rows
// (sg_mask_bits_ids_count / _fill) and the union of the members' ids as maximal runs (sg_stitch_union_count /
// _fill).  The rules are stated in include/softgroup_hip.h; the reference only cuts blocks offline
// (dataset/stpls3d/prepare_data_inst_instance_stpls3d.py) and evaluates each as a scene of its own.
//
// Everything here is integer or IEEE double arithmetic (-ffp-contract=off), selection by integer atomics only
// (atomicCAS on a key, atomicOr on bits): two calls on the same input give the same bytes.  The order inside a
// tile and inside an object comes from the stable radix sort, never from the order in which atomics arrive.
//
// Bounds that do not depend on the data: every probe loop ends after kTaCap probes, every binary search after 32
// steps, the component rounds after G; every index read from memory is range-checked before it addresses
// anything.  No workgroup waits for another one: where grids must agree there is another launch.
#include "common.h"
#include "cross_links.h"
#include "radix_sort.h"
#include "scan.h"

namespace sg {

constexpr int kStBlock = 256;
constexpr int kTaCap = 1 << 18;                      // slots of the cell table (a power of two, 4 x the tile limit)
constexpr int kTaMaxTiles = 65535;
constexpr int kTaListCap = 65536;
constexpr double kTaCellLimit = 1073741824.0;        // |cell| < 2^30
constexpr int32_t kTaBias = 1 << 30;
constexpr uint64_t kTaEmpty = ~0ull;
constexpr int kTaFlagInvalid = 1, kTaFlagTiles = 2;
constexpr int kStMaxInst = 16384;
constexpr int kCcBlock = 1024;
constexpr uint32_t kIdsTrash = 0xFFFFu;               // "no object": above every object number, inside 16 sort bits

// ---- tiles -----------------------------------------------------------------------------------------------------
struct TaArgs {
  const float *xyz;
  int64_t n;
  double size, margin, ox, oy;
  int32_t *meta;                    // [0] tiles, [1] flags, [2] entries of tile_points
  unsigned long long *key;          // [kTaCap]    biased (cy, cx) of the slot's cell, all ones = free
  int32_t *tile_of_slot;            // [kTaCap]
  unsigned long long *list;         // [kTaListCap] the cells in slot order
  int32_t *list_slot;               // [kTaListCap]
  unsigned long long *sorted;       // [kTaListCap] the cells in ascending (cy, cx) order
  unsigned long long *member;       // [n] four 16-bit tile numbers (0xFFFF = none), the core tile in the low one
  int32_t *ent_off;                 // [n] exclusive count of memberships below point i
};

__device__ __forceinline__ bool ta_cell(double x, double o, double size, int32_t *c) {
  const double f = floor((x - o) / size);
  const bool in = fabs(f) < kTaCellLimit;             // (NaN / inf fail the comparison)
  *c = in ? static_cast<int32_t>(f) : 0;
  return in;
}

__device__ __forceinline__ unsigned long long ta_key(int32_t cx, int32_t cy) {
  return (static_cast<unsigned long long>(static_cast<uint32_t>(cy + kTaBias)) << 32) |
         static_cast<uint32_t>(cx + kTaBias);
}

// -1 / +1: the neighbouring cell the coordinate also belongs to, 0: none
__device__ __forceinline__ int ta_side(double x, double o, double size, double margin, int32_t c) {
  if (!(margin > 0.0)) return 0;
  const double lo = o + static_cast<double>(c) * size;
  const double hi = o + static_cast<double>(c + 1) * size;
  if (x < lo + margin) return -1;
  if (x >= hi - margin) return 1;
  return 0;
}

__global__ void __launch_bounds__(kStBlock) ta_validate_kernel(TaArgs a) {
  int bad = 0;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kStBlock) + threadIdx.x; i < a.n;
       i += static_cast<int64_t>(gridDim.x) * kStBlock) {
    const float *p = a.xyz + 3 * i;
    int32_t c;
    if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) || !ta_cell(p[0], a.ox, a.size, &c) ||
        !ta_cell(p[1], a.oy, a.size, &c))
      bad = kTaFlagInvalid;
  }
  if (bad) atomicOr(a.meta + 1, bad);
}

__global__ void __launch_bounds__(kStBlock) ta_insert_kernel(TaArgs a) {
  if (a.meta[1] != 0) return;                                     // invalid input: no table is touched
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kStBlock) + threadIdx.x; i < a.n;
       i += static_cast<int64_t>(gridDim.x) * kStBlock) {
    const float *p = a.xyz + 3 * i;
    int32_t cx, cy;
    if (!ta_cell(p[0], a.ox, a.size, &cx) || !ta_cell(p[1], a.oy, a.size, &cy)) continue;
    const unsigned long long k = ta_key(cx, cy);
    uint32_t s = static_cast<uint32_t>(mix64(k)) & (kTaCap - 1);
    bool placed = false;
    for (int probe = 0; probe < kTaCap; ++probe) {
      unsigned long long cur = __atomic_load_n(&a.key[s], __ATOMIC_RELAXED);      // (most points find their cell here)
      if (cur == kTaEmpty) cur = atomicCAS(&a.key[s], kTaEmpty, k);
      if (cur == kTaEmpty || cur == k) {
        placed = true;
        break;
      }
      s = (s + 1) & (kTaCap - 1);
    }
    if (!placed) atomicOr(a.meta + 1, kTaFlagTiles);              // (a full table: far more cells than tiles allowed)
  }
}

// rank of every cell among all cells = its tile number (the cells are distinct)
__global__ void __launch_bounds__(kStBlock) ta_rank_kernel(TaArgs a) {
  const int32_t t_raw = a.meta[0];
  if (a.meta[1] != 0) return;
  if (t_raw > kTaMaxTiles || t_raw < 0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(a.meta + 1, kTaFlagTiles);
    return;
  }
  for (int i = blockIdx.x * kStBlock + threadIdx.x; i < t_raw; i += gridDim.x * kStBlock) {
    const unsigned long long k = a.list[i];
    int r = 0;
    for (int j = 0; j < t_raw; ++j) r += a.list[j] < k ? 1 : 0;
    a.sorted[r] = k;
    const int32_t s = a.list_slot[i];
    if (s >= 0 && s < kTaCap) a.tile_of_slot[s] = r;
  }
}

// tile number of a cell, 0xFFFF when the cell is not a tile
__device__ __forceinline__ uint32_t ta_lookup(const TaArgs &a, int32_t cx, int32_t cy, int32_t n_tiles) {
  const unsigned long long k = ta_key(cx, cy);
  uint32_t s = static_cast<uint32_t>(mix64(k)) & (kTaCap - 1);
  for (int probe = 0; probe < kTaCap; ++probe) {
    const unsigned long long cur = a.key[s];
    if (cur == kTaEmpty) return 0xFFFFu;
    if (cur == k) {
      const int32_t t = a.tile_of_slot[s];
      return t >= 0 && t < n_tiles ? static_cast<uint32_t>(t) : 0xFFFFu;
    }
    s = (s + 1) & (kTaCap - 1);
  }
  return 0xFFFFu;
}

__global__ void __launch_bounds__(kStBlock) ta_member_kernel(TaArgs a) {
  const bool bad = a.meta[1] != 0;
  const int32_t n_tiles = a.meta[0];
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kStBlock) + threadIdx.x; i < a.n;
       i += static_cast<int64_t>(gridDim.x) * kStBlock) {
    unsigned long long m = kTaEmpty;
    const float *p = a.xyz + 3 * i;
    int32_t cx, cy;
    if (!bad && ta_cell(p[0], a.ox, a.size, &cx) && ta_cell(p[1], a.oy, a.size, &cy)) {
      const int dx = ta_side(p[0], a.ox, a.size, a.margin, cx), dy = ta_side(p[1], a.oy, a.size, a.margin, cy);
      const uint32_t t0 = ta_lookup(a, cx, cy, n_tiles);
      const uint32_t t1 = dx != 0 ? ta_lookup(a, cx + dx, cy, n_tiles) : 0xFFFFu;      // |c| < 2^30: no overflow
      const uint32_t t2 = dy != 0 ? ta_lookup(a, cx, cy + dy, n_tiles) : 0xFFFFu;
      const uint32_t t3 = dx != 0 && dy != 0 ? ta_lookup(a, cx + dx, cy + dy, n_tiles) : 0xFFFFu;
      m = static_cast<unsigned long long>(t0) | (static_cast<unsigned long long>(t1) << 16) |
          (static_cast<unsigned long long>(t2) << 32) | (static_cast<unsigned long long>(t3) << 48);
    }
    a.member[i] = m;
  }
}

__device__ __forceinline__ int ta_mult(unsigned long long m) {
  int c = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) c += ((m >> (16 * k)) & 0xFFFFu) != 0xFFFFu ? 1 : 0;
  return c;
}

__global__ void __launch_bounds__(kStBlock) ta_entries_kernel(TaArgs a, int32_t n_tiles, int64_t total,
                                                             uint32_t *__restrict__ keys, int32_t *__restrict__ vals,
                                                             int32_t *__restrict__ core_tile) {
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kStBlock) + threadIdx.x; i < a.n;
       i += static_cast<int64_t>(gridDim.x) * kStBlock) {
    const unsigned long long m = a.member[i];
    int64_t at = a.ent_off[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t t = static_cast<uint32_t>(m >> (16 * k)) & 0xFFFFu;
      if (k == 0) core_tile[i] = static_cast<int32_t>(t) < n_tiles ? static_cast<int32_t>(t) : -1;
      if (static_cast<int32_t>(t) >= n_tiles) continue;
      if (at >= 0 && at < total) keys[at] = t, vals[at] = static_cast<int32_t>(i);
      ++at;
    }
  }
}

__global__ void __launch_bounds__(kStBlock) ta_emit_kernel(const uint32_t *__restrict__ keys,
                                                          const int32_t *__restrict__ vals, int64_t total, int64_t n,
                                                          int32_t n_tiles, const unsigned long long *__restrict__ sorted,
                                                          int32_t *__restrict__ tile_cells, int64_t *__restrict__ tile_off,
                                                          int32_t *__restrict__ tile_points) {
  for (int64_t e = blockIdx.x * static_cast<int64_t>(kStBlock) + threadIdx.x; e < total;
       e += static_cast<int64_t>(gridDim.x) * kStBlock) {
    const uint32_t t = keys[e];
    const int32_t p = vals[e];
    tile_points[e] = p >= 0 && p < n ? p : 0;
    if (static_cast<int32_t>(t) < n_tiles && (e == 0 || keys[e - 1] != t)) tile_off[t] = e;
  }
  for (int64_t t = blockIdx.x * static_cast<int64_t>(kStBlock) + threadIdx.x; t <= n_tiles;
       t += static_cast<int64_t>(gridDim.x) * kStBlock) {
    if (t == n_tiles) {
      tile_off[t] = total;
    } else {
      const unsigned long long k = sorted[t];
      tile_cells[2 * t] = static_cast<int32_t>(static_cast<uint32_t>(k)) - kTaBias;            // cx
      tile_cells[2 * t + 1] = static_cast<int32_t>(static_cast<uint32_t>(k >> 32)) - kTaBias;      // cy
    }
  }
}

__global__ void __launch_bounds__(kStBlock) ta_core_pos_kernel(const uint32_t *__restrict__ keys,
                                                              const int32_t *__restrict__ vals, int64_t total, int64_t n,
                                                              int32_t n_tiles, const int64_t *__restrict__ tile_off,
                                                              const int32_t *__restrict__ core_tile,
                                                              int32_t *__restrict__ core_pos) {
  for (int64_t e = blockIdx.x * static_cast<int64_t>(kStBlock) + threadIdx.x; e < total;
       e += static_cast<int64_t>(gridDim.x) * kStBlock) {
    const uint32_t t = keys[e];
    const int32_t p = vals[e];
    if (static_cast<int32_t>(t) >= n_tiles || p < 0 || p >= n) continue;
    if (core_tile[p] == static_cast<int32_t>(t)) core_pos[p] = static_cast<int32_t>(e - tile_off[t]);
  }
}

static size_t ta_bytes(int64_t n) {
  const size_t nn = static_cast<size_t>(n > 0 ? n : 1);
  return align_up(static_cast<size_t>(kTaCap) * 8) + align_up(static_cast<size_t>(kTaCap) * 4) +
         2 * align_up(static_cast<size_t>(kTaListCap) * 8) + align_up(static_cast<size_t>(kTaListCap) * 4) +
         align_up(nn * 8) + align_up(nn * 4) + align_up(scan_workspace_bytes(kTaCap)) +
         align_up(scan_workspace_bytes(static_cast<int64_t>(nn))) + 256;
}

struct TaWs {
  void *scan_t, *scan_n;
  size_t scan_t_bytes, scan_n_bytes;
};

static bool ta_carve(void *ws, size_t ws_bytes, int64_t n, TaArgs *a, TaWs *w) {
  if (ws == nullptr || ws_bytes < ta_bytes(n)) return false;
  const size_t nn = static_cast<size_t>(n > 0 ? n : 1);
  Workspace b(ws, ws_bytes);
  a->key = b.take<unsigned long long>(kTaCap);
  a->tile_of_slot = b.take<int32_t>(kTaCap);
  a->list = b.take<unsigned long long>(kTaListCap);
  a->sorted = b.take<unsigned long long>(kTaListCap);
  a->list_slot = b.take<int32_t>(kTaListCap);
  a->member = b.take<unsigned long long>(nn);
  a->ent_off = b.take<int32_t>(nn);
  w->scan_t_bytes = scan_workspace_bytes(kTaCap);
  w->scan_t = b.take<char>(w->scan_t_bytes);
  w->scan_n_bytes = scan_workspace_bytes(static_cast<int64_t>(nn));
  w->scan_n = b.take<char>(w->scan_n_bytes);
  return w->scan_n != nullptr;
}

static bool ta_args_ok(int n, double size, double margin, double ox, double oy) {
  const double big = 1.7976931348623157e308;
  return n >= 0 && n < (1 << 29) && size > 0.0 && size <= big && margin >= 0.0 && margin <= size / 2 &&
         fabs(ox) <= big && fabs(oy) <= big;
}

// ---- shared points of two ascending lists ---------------------------------------------------------------------
__global__ void __launch_bounds__(kStBlock) shared_find_kernel(const int32_t *__restrict__ a, int n_a,
                                                              const int32_t *__restrict__ b, int n_b,
                                                              int32_t *__restrict__ found) {
  for (int i = blockIdx.x * kStBlock + threadIdx.x; i < n_a; i += gridDim.x * kStBlock) {
    const int32_t v = a[i];
    int lo = 0, hi = n_b;                                          // lower bound: at most 32 halvings
    for (int step = 0; step < 32 && lo < hi; ++step) {
      const int mid = lo + ((hi - lo) >> 1);
      if (b[mid] < v) lo = mid + 1; else hi = mid;
    }
    found[i] = lo < n_b && b[lo] == v ? lo : -1;
  }
}

// ---- rectangular intersections and links ----------------------------------------------------------------------
// (ClArgs: cross_links.h)
// One workgroup per pair of 4-row tiles (ti of a, tj of b), lane = word: 8 coalesced loads, 16 popcount(a & b)
// and 8 population accumulators per lane and step; the four waves split the word range and meet in LDS.
__global__ void __launch_bounds__(kStBlock) cross_links_kernel(ClArgs a) {
  __shared__ int part[4][kClTile * kClTile + 2 * kClTile];
  const int tid = threadIdx.x;
  const int64_t nta = (a.n_a + kClTile - 1) / kClTile, ntb = (a.n_b + kClTile - 1) / kClTile;
  const int tail = static_cast<int>(a.n_bits & 31);
  constexpr int kAcc = kClTile * kClTile + 2 * kClTile;
  for (int64_t p = blockIdx.x; p < nta * ntb; p += gridDim.x) {      // (block-uniform)
    const int ti = static_cast<int>(p / ntb), tj = static_cast<int>(p - ti * ntb);
    if (a.symmetric && ti > tj) continue;                           // (block-uniform, before the barriers)
    int ra[kClTile], rb[kClTile];
#pragma unroll
    for (int k = 0; k < kClTile; ++k) {
      ra[k] = min(ti * kClTile + k, a.n_a - 1);                     // (a ragged tile repeats its last row; not used below)
      rb[k] = min(tj * kClTile + k, a.n_b - 1);
    }
    int acc[kAcc];
#pragma unroll
    for (int x = 0; x < kAcc; ++x) acc[x] = 0;
    for (int64_t w = tid; w < a.words; w += kStBlock) {
      uint32_t va[kClTile], vb[kClTile];
#pragma unroll
      for (int k = 0; k < kClTile; ++k) {
        va[k] = a.bits_a[static_cast<int64_t>(ra[k]) * a.words + w];
        vb[k] = a.bits_b[static_cast<int64_t>(rb[k]) * a.words + w];
      }
      if (w == a.words - 1 && tail) {                               // bits at and beyond n_bits are ignored, on both sides
#pragma unroll
        for (int k = 0; k < kClTile; ++k) va[k] &= (1u << tail) - 1u, vb[k] &= (1u << tail) - 1u;
      }
#pragma unroll
      for (int k = 0; k < kClTile; ++k) {
#pragma unroll
        for (int l = 0; l < kClTile; ++l) acc[k * kClTile + l] += __popc(va[k] & vb[l]);
        acc[kClTile * kClTile + k] += __popc(va[k]);
        acc[kClTile * kClTile + kClTile + k] += __popc(vb[k]);
      }
    }
#pragma unroll
    for (int x = 0; x < kAcc; ++x) {
      const int v = wave_sum(acc[x]);
      if ((tid & 63) == 0) part[tid >> 6][x] = v;
    }
    __syncthreads();
    if (tid < kClTile * kClTile) {
      const int k = tid / kClTile, l = tid % kClTile;
      const int i = ti * kClTile + k, j = tj * kClTile + l;
      if (i < a.n_a && j < a.n_b) {
        const int xa = kClTile * kClTile + k, xb = kClTile * kClTile + kClTile + l;
        const int inter = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
        const int64_t ca = part[0][xa] + part[1][xa] + part[2][xa] + part[3][xa];
        const int64_t cb = part[0][xb] + part[1][xb] + part[2][xb] + part[3][xb];
        if (a.inter_out != nullptr) a.inter_out[static_cast<int64_t>(i) * a.n_b + j] = inter;
        if (a.cnt_a_out != nullptr && j == 0) a.cnt_a_out[i] = static_cast<int32_t>(ca);
        if (a.cnt_b_out != nullptr && i == 0) a.cnt_b_out[j] = static_cast<int32_t>(cb);
        const int64_t den = a.measure == 0 ? ca + cb - inter : (ca < cb ? ca : cb);
        const int64_t gi = static_cast<int64_t>(a.base_a) + i, gj = static_cast<int64_t>(a.base_b) + j;
        if (a.adj != nullptr && gi < a.n_total && gj < a.n_total && gi != gj && a.labels_a[i] == a.labels_b[j] &&
            (a.group_a == nullptr || a.group_a[i] != a.group_b[j]) && inter >= a.min_shared && den > 0 &&
            static_cast<double>(inter) / static_cast<double>(den) > a.thr) {
          atomicOr(&a.adj[gi * a.nw + (gj >> 5)], 1u << (gj & 31));
          atomicOr(&a.adj[gj * a.nw + (gi >> 5)], 1u << (gi & 31));
        }
      }
    }
    __syncthreads();
  }
}

void cross_links_launch(const ClArgs &a, int max_blocks, hipStream_t stream) {
  const int64_t nta = (a.n_a + kClTile - 1) / kClTile, ntb = (a.n_b + kClTile - 1) / kClTile;
  cross_links_kernel<<<grid_for(nta * ntb, 1, max_blocks), kStBlock, 0, stream>>>(a);
}

// ---- connected components -------------------------------------------------------------------------------------
// One workgroup, the labels in LDS (G <= 16384 values below 2^16).  A round takes for every node the smallest
// label among itself and its neighbours, then jumps label[g] = label[label[g]].  Labels only fall, every value is
// a member of the node's component and label[g] <= g, so stale reads inside a round cost rounds, not
// correctness; a round whose first half changes nothing has every component at its smallest member.
__global__ void __launch_bounds__(kCcBlock) components_kernel(const uint32_t *__restrict__ adj, int n, int nw,
                                                             int32_t *__restrict__ comp) {
  __shared__ uint16_t label[kStMaxInst];
  __shared__ int changed;
  const int tid = threadIdx.x;
  for (int g = tid; g < n; g += kCcBlock) label[g] = static_cast<uint16_t>(g);
  if (tid == 0) changed = 0;
  __syncthreads();
  for (int round = 0; round <= n; ++round) {                        // (every branch around a barrier is block-uniform)
    bool mine = false;
    for (int g = tid; g < n; g += kCcBlock) {
      uint32_t best = label[g];
      const uint32_t *row = adj + static_cast<int64_t>(g) * nw;
      for (int w = 0; w < nw; ++w) {
        uint32_t x = row[w];
        if (w == nw - 1 && (n & 31)) x &= (1u << (n & 31)) - 1u;
        for (; x; x &= x - 1) {                                     // at most 32 bits
          const int h = 32 * w + (__ffs(x) - 1);
          const uint32_t lh = label[h];
          best = lh < best ? lh : best;
        }
      }
      if (best < label[g]) label[g] = static_cast<uint16_t>(best), mine = true;
    }
    if (mine) changed = 1;
    __syncthreads();
    const int any = changed;
    __syncthreads();
    if (!any) break;
    if (tid == 0) changed = 0;
    for (int g = tid; g < n; g += kCcBlock) {
      const uint32_t l = label[g];
      const uint32_t ll = l < static_cast<uint32_t>(n) ? label[l] : l;
      if (ll < l) label[g] = static_cast<uint16_t>(ll);
    }
    __syncthreads();
  }
  for (int g = tid; g < n; g += kCcBlock) comp[g] = label[g];
}

// ---- set bits of tile rows as global ids ----------------------------------------------------------------------
__global__ void __launch_bounds__(kStBlock) ids_count_kernel(const uint32_t *__restrict__ bits, int n, int64_t n_bits,
                                                            int64_t words, const uint8_t *__restrict__ core,
                                                            int32_t *__restrict__ cnt, int32_t *__restrict__ core_cnt) {
  __shared__ int s_c[4], s_k[4];
  const int tid = threadIdx.x;
  const int tail = static_cast<int>(n_bits & 31);
  for (int r = blockIdx.x; r < n; r += gridDim.x) {
    const uint32_t *row = bits + static_cast<int64_t>(r) * words;
    int c = 0, k = 0;
    for (int64_t w = tid; w < words; w += kStBlock) {
      uint32_t x = row[w];
      if (w == words - 1 && tail) x &= (1u << tail) - 1u;
      c += __popc(x);
      if (core != nullptr)
        for (; x; x &= x - 1) k += core[32 * w + (__ffs(x) - 1)] != 0 ? 1 : 0;
    }
    c = wave_sum(c), k = wave_sum(k);
    if ((tid & 63) == 0) s_c[tid >> 6] = c, s_k[tid >> 6] = k;
    __syncthreads();
    if (tid == 0) {
      cnt[r] = s_c[0] + s_c[1] + s_c[2] + s_c[3];
      core_cnt[r] = s_k[0] + s_k[1] + s_k[2] + s_k[3];
    }
    __syncthreads();
  }
}

// One workgroup per row: 256 words per step, the position of a word's first id = the row's offset + the block
// scan of the populations (position order = bit order, nothing depends on arrival).
__global__ void __launch_bounds__(kStBlock) ids_fill_kernel(const uint32_t *__restrict__ bits, int n, int64_t n_bits,
                                                           int64_t words, const int32_t *__restrict__ map,
                                                           int64_t n_points, const int64_t *__restrict__ row_off,
                                                           const int32_t *__restrict__ row_key,
                                                           int32_t *__restrict__ ids, uint32_t *__restrict__ keys,
                                                           int64_t capacity, int32_t *__restrict__ meta) {
  __shared__ int lds4[4];
  const int tid = threadIdx.x;
  const int tail = static_cast<int>(n_bits & 31);
  for (int r = blockIdx.x; r < n; r += gridDim.x) {                 // (block-uniform)
    const uint32_t *row = bits + static_cast<int64_t>(r) * words;
    const int32_t rk = row_key[r];
    const uint32_t key = rk >= 0 ? static_cast<uint32_t>(rk) : kIdsTrash;
    int64_t run = row_off[r];
    for (int64_t w0 = 0; w0 < words; w0 += kStBlock) {
      const int64_t w = w0 + tid;
      uint32_t x = w < words ? row[w] : 0u;
      if (w == words - 1 && tail) x &= (1u << tail) - 1u;
      const int c = __popc(x);
      int total = 0;
      const int incl = block_incl_scan_256(c, lds4, &total);
      int64_t at = run + incl - c;
      for (; x; x &= x - 1, ++at) {
        const int64_t pos = 32 * w + (__ffs(x) - 1);
        const int32_t id = map[pos];
        const bool ok = id >= 0 && id < n_points;
        if (!ok) atomicOr(meta, 1);
        if (at >= 0 && at < capacity) ids[at] = ok ? id : 0, keys[at] = ok ? key : kIdsTrash;
      }
      run += total;
    }
  }
}

// ---- union: sorted (object, id) pairs -> maximal runs ---------------------------------------------------------
struct UnArgs {
  const uint32_t *k;      // sorted object numbers (>= n_obj: not part of any object)
  const int32_t *v;       // ids, ascending inside an object
  int64_t total;
  int n_obj;
};

__device__ __forceinline__ int un_is_start(const UnArgs &u, int64_t e) {
  const uint32_t k = u.k[e];
  if (k >= static_cast<uint32_t>(u.n_obj)) return 0;
  if (e == 0 || u.k[e - 1] != k) return 1;
  return static_cast<int64_t>(u.v[e]) > static_cast<int64_t>(u.v[e - 1]) + 1 ? 1 : 0;      // equal ids collapse, +1 continues
}

__device__ __forceinline__ int un_is_end(const UnArgs &u, int64_t e) {
  const uint32_t k = u.k[e];
  if (k >= static_cast<uint32_t>(u.n_obj)) return 0;
  if (e == u.total - 1 || u.k[e + 1] != k) return 1;
  return static_cast<int64_t>(u.v[e + 1]) > static_cast<int64_t>(u.v[e]) + 1 ? 1 : 0;
}

__global__ void __launch_bounds__(kStBlock) un_bounds_kernel(UnArgs u, const int32_t *__restrict__ ridx,
                                                            const int32_t *__restrict__ total_runs,
                                                            int64_t *__restrict__ bounds) {
  for (int o = blockIdx.x * kStBlock + threadIdx.x; o <= u.n_obj; o += gridDim.x * kStBlock) {
    int64_t lo = 0, hi = u.total;                                   // first entry of an object >= o
    for (int step = 0; step < 32 && lo < hi; ++step) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (u.k[mid] < static_cast<uint32_t>(o)) lo = mid + 1; else hi = mid;
    }
    bounds[o] = (o < u.n_obj && lo < u.total) ? ridx[lo] : *total_runs;
  }
}

__global__ void __launch_bounds__(kStBlock) un_fill_kernel(UnArgs u, const int32_t *__restrict__ ridx,
                                                          int32_t *__restrict__ starts, int32_t *__restrict__ ends,
                                                          int64_t capacity) {
  for (int64_t e = blockIdx.x * static_cast<int64_t>(kStBlock) + threadIdx.x; e < u.total;
       e += static_cast<int64_t>(gridDim.x) * kStBlock) {
    const int s = un_is_start(u, e), t = un_is_end(u, e);
    const int64_t r = ridx[e];
    if (s && r >= 0 && r < capacity) starts[r] = u.v[e];
    const int64_t q = r + s - 1;                                    // the run that ends here started at or before e
    if (t && q >= 0 && q < capacity) ends[q] = u.v[e] + 1;
  }
}

__global__ void __launch_bounds__(kStBlock) un_copy_kernel(const int32_t *__restrict__ ids,
                                                          const uint32_t *__restrict__ keys, int64_t total, int n_obj,
                                                          int64_t n_points, int32_t *__restrict__ ids_out,
                                                          uint32_t *__restrict__ keys_out) {
  for (int64_t e = blockIdx.x * static_cast<int64_t>(kStBlock) + threadIdx.x; e < total;
       e += static_cast<int64_t>(gridDim.x) * kStBlock) {
    const int32_t id = ids[e];
    const uint32_t k = keys[e];
    const bool ok = id >= 0 && id < n_points && k < static_cast<uint32_t>(n_obj);
    ids_out[e] = ok ? id : 0;
    keys_out[e] = ok ? k : kIdsTrash;
  }
}

struct UnWs {
  uint32_t *keys;
  int32_t *ids, *ridx, *total_runs;
  void *sort, *scan;
  size_t sort_bytes, scan_bytes;
};

static bool un_in_range(int64_t total, int n_obj, int64_t n_points) {
  return total >= 0 && total < (1LL << 31) && n_obj >= 0 && n_obj <= kStMaxInst && n_points >= 0 &&
         n_points < (1LL << 31);
}

static size_t un_bytes(int64_t total) {
  const size_t t = static_cast<size_t>(total > 0 ? total : 1);
  return 3 * align_up(t * 4) + align_up(64 * 4) + align_up(radix_sort_workspace_bytes(total)) +
         align_up(scan_workspace_bytes(total)) + 256;
}

static bool un_carve(void *ws, size_t ws_bytes, int64_t total, UnWs *m) {
  if (ws == nullptr || ws_bytes < un_bytes(total)) return false;
  const size_t t = static_cast<size_t>(total > 0 ? total : 1);
  Workspace a(ws, ws_bytes);
  m->keys = a.take<uint32_t>(t);
  m->ids = a.take<int32_t>(t);
  m->ridx = a.take<int32_t>(t);
  m->total_runs = a.take<int32_t>(64);
  m->sort_bytes = radix_sort_workspace_bytes(total);
  m->sort = a.take<char>(m->sort_bytes);
  m->scan_bytes = scan_workspace_bytes(total);
  m->scan = a.take<char>(m->scan_bytes);
  return m->scan != nullptr;
}

static int bit_length(int64_t v) {
  int b = 0;
  while (v > 0) ++b, v >>= 1;
  return b;
}

}  // namespace sg

using namespace sg;

extern "C" {

size_t sg_tile_assign_workspace_bytes(int n) { return n < 0 || n >= (1 << 29) ? 0 : ta_bytes(n); }

size_t sg_tile_assign_fill_workspace_bytes(int64_t total) {
  if (total < 0 || total >= (1LL << 31)) return 0;
  const size_t t = static_cast<size_t>(total > 0 ? total : 1);
  return 2 * align_up(t * 4) + align_up(radix_sort_workspace_bytes(total)) + 256;
}

int sg_tile_assign_count(const float *xyz, int n, double size, double margin, double ox, double oy, int32_t *meta,
                         void *ws, size_t ws_bytes, sg_stream_t stream_) {
  if (n >= (1 << 29)) {
    set_error("sg_tile_assign_count: %d points outside the supported range (n < 2^29)", n);
    return SG_ERR_UNSUPPORTED;
  }
  SG_REQUIRE(ta_args_ok(n, size, margin, ox, oy) && meta != nullptr && (n == 0 || xyz != nullptr),
             "sg_tile_assign_count: bad arguments (n=%d size=%g margin=%g)", n, size, margin);
  TaArgs a;
  TaWs w;
  if (!ta_carve(ws, ws_bytes, n, &a, &w)) {
    set_error("sg_tile_assign_count: workspace too small");
    return SG_ERR_WORKSPACE;
  }
  a.xyz = xyz, a.n = n, a.size = size, a.margin = margin, a.ox = ox, a.oy = oy, a.meta = meta;
  hipStream_t stream = as_stream(stream_);
  FillList f;
  f.add(meta, 16, 0);
  f.add(a.key, static_cast<size_t>(kTaCap) * 8, 0xff);
  f.add(a.tile_of_slot, static_cast<size_t>(kTaCap) * 4, 0xff);
  fill_many(f, stream);
  if (n == 0) return check_launch("sg_tile_assign_count");
  const int grid = grid_for(n, kStBlock, 4096);
  ta_validate_kernel<<<grid, kStBlock, 0, stream>>>(a);
  ta_insert_kernel<<<grid, kStBlock, 0, stream>>>(a);
  const unsigned long long *key = a.key;
  unsigned long long *list = a.list;
  int32_t *list_slot = a.list_slot;
  int rc = exclusive_scan([key] __device__(int64_t s) { return key[s] != kTaEmpty ? 1 : 0; },
                          [key, list, list_slot] __device__(int64_t s, int v) {
                            if (key[s] != kTaEmpty && v >= 0 && v < kTaListCap) list[v] = key[s], list_slot[v] = static_cast<int32_t>(s);
                          },
                          kTaCap, meta, w.scan_t, w.scan_t_bytes, stream);
  if (rc != SG_OK) return rc;
  ta_rank_kernel<<<grid_for(kTaListCap, kStBlock, 256), kStBlock, 0, stream>>>(a);
  ta_member_kernel<<<grid, kStBlock, 0, stream>>>(a);
  const unsigned long long *member = a.member;
  int32_t *ent_off = a.ent_off;
  rc = exclusive_scan([member] __device__(int64_t i) { return ta_mult(member[i]); },
                      [ent_off] __device__(int64_t i, int v) { ent_off[i] = v; }, n, meta + 2, w.scan_n,
                      w.scan_n_bytes, stream);
  if (rc != SG_OK) return rc;
  return check_launch("sg_tile_assign_count");
}

int sg_tile_assign_fill(const float *xyz, int n, double size, double margin, double ox, double oy, int n_tiles,
                        int64_t total, int32_t *tile_cells, int64_t *tile_off, int32_t *tile_points,
                        int32_t *core_tile, int32_t *core_pos, const void *ws, size_t ws_bytes, void *ws2,
                        size_t ws2_bytes, sg_stream_t stream_) {
  SG_REQUIRE(ta_args_ok(n, size, margin, ox, oy) && n_tiles >= 0 && n_tiles <= kTaMaxTiles && total >= n &&
                 total <= 4 * static_cast<int64_t>(n) && tile_off != nullptr,
             "sg_tile_assign_fill: bad arguments (n=%d tiles=%d total=%lld)", n, n_tiles, static_cast<long long>(total));
  SG_REQUIRE(n == 0 || (xyz != nullptr && tile_cells != nullptr && tile_points != nullptr && core_tile != nullptr &&
                        core_pos != nullptr && n_tiles >= 1),
             "sg_tile_assign_fill: null array");
  TaArgs a;
  TaWs w;
  if (!ta_carve(const_cast<void *>(ws), ws_bytes, n, &a, &w) || ws2 == nullptr ||
      ws2_bytes < sg_tile_assign_fill_workspace_bytes(total)) {
    set_error("sg_tile_assign_fill: workspace too small");
    return SG_ERR_WORKSPACE;
  }
  a.xyz = xyz, a.n = n, a.size = size, a.margin = margin, a.ox = ox, a.oy = oy, a.meta = nullptr;
  hipStream_t stream = as_stream(stream_);
  FillList f;
  f.add(tile_off, static_cast<size_t>(n_tiles + 1) * 8, 0);
  if (n > 0) f.add(core_pos, static_cast<size_t>(n) * 4, 0xff);
  fill_many(f, stream);
  if (n == 0) return check_launch("sg_tile_assign_fill");
  const size_t t = static_cast<size_t>(total);
  Workspace b(ws2, ws2_bytes);
  uint32_t *keys = b.take<uint32_t>(t);
  int32_t *vals = b.take<int32_t>(t);
  const size_t sort_bytes = radix_sort_workspace_bytes(total);
  void *sort_ws = b.take<char>(sort_bytes);
  SG_REQUIRE(sort_ws != nullptr, "sg_tile_assign_fill: workspace too small");
  ta_entries_kernel<<<grid_for(n, kStBlock, 4096), kStBlock, 0, stream>>>(a, n_tiles, total, keys, vals, core_tile);
  uint32_t *ks;
  int32_t *vs;
  const int rc = radix_sort_pairs(keys, vals, total, 16, sort_ws, sort_bytes, stream, &ks, &vs);
  if (rc != SG_OK) return rc;
  const int grid = grid_for(total, kStBlock, 4096);
  ta_emit_kernel<<<grid, kStBlock, 0, stream>>>(ks, vs, total, n, n_tiles, a.sorted, tile_cells, tile_off, tile_points);
  ta_core_pos_kernel<<<grid, kStBlock, 0, stream>>>(ks, vs, total, n, n_tiles, tile_off, core_tile, core_pos);
  return check_launch("sg_tile_assign_fill");
}

size_t sg_tile_shared_workspace_bytes(int n_a) {
  if (n_a < 0) return 0;
  return align_up(static_cast<size_t>(n_a > 0 ? n_a : 1) * 4) + align_up(scan_workspace_bytes(n_a)) + 256;
}

int sg_tile_shared(const int32_t *a, int n_a, const int32_t *b, int n_b, int32_t *pos_a, int32_t *pos_b,
                   int32_t *count, void *ws, size_t ws_bytes, sg_stream_t stream_) {
  SG_REQUIRE(n_a >= 0 && n_b >= 0 && count != nullptr, "sg_tile_shared: bad arguments (n_a=%d n_b=%d)", n_a, n_b);
  SG_REQUIRE((n_a == 0 || a != nullptr) && (n_b == 0 || b != nullptr) &&
                 (n_a == 0 || n_b == 0 || (pos_a != nullptr && pos_b != nullptr)),
             "sg_tile_shared: null array");
  if (ws == nullptr || ws_bytes < sg_tile_shared_workspace_bytes(n_a)) {
    set_error("sg_tile_shared: workspace too small");
    return SG_ERR_WORKSPACE;
  }
  hipStream_t stream = as_stream(stream_);
  if (n_a == 0 || n_b == 0) {
    FillList f;
    f.add(count, 4, 0);
    fill_many(f, stream);
    return check_launch("sg_tile_shared");
  }
  Workspace w(ws, ws_bytes);
  int32_t *found = w.take<int32_t>(n_a);
  const size_t sbytes = scan_workspace_bytes(n_a);
  void *sws = w.take<char>(sbytes);
  SG_REQUIRE(sws != nullptr, "sg_tile_shared: workspace too small");
  shared_find_kernel<<<grid_for(n_a, kStBlock, 4096), kStBlock, 0, stream>>>(a, n_a, b, n_b, found);
  const int cap = n_a < n_b ? n_a : n_b;
  const int32_t *fnd = found;
  const int rc = exclusive_scan([fnd] __device__(int64_t i) { return fnd[i] >= 0 ? 1 : 0; },
                                [fnd, pos_a, pos_b, cap] __device__(int64_t i, int v) {
                                  if (fnd[i] >= 0 && v >= 0 && v < cap) pos_a[v] = static_cast<int32_t>(i), pos_b[v] = fnd[i];
                                },
                                n_a, count, sws, sbytes, stream);
  if (rc != SG_OK) return rc;
  return check_launch("sg_tile_shared");
}

int sg_mask_cross_links(const uint32_t *bits_a, int n_a, const uint32_t *bits_b, int n_b, int64_t n_bits,
                        const int32_t *labels_a, const int32_t *labels_b, int base_a, int base_b, int n_total,
                        double thr, int measure, int min_shared, uint32_t *adj, int32_t *inter_out,
                        int32_t *cnt_a_out, int32_t *cnt_b_out, sg_stream_t stream_) {
  if (n_total < 0 || n_total > kStMaxInst || n_bits < 0 || n_bits >= (1LL << 31)) {
    set_error("sg_mask_cross_links: %d instances, %lld bits outside the supported range (<= %d, < 2^31)", n_total,
              static_cast<long long>(n_bits), kStMaxInst);
    return SG_ERR_UNSUPPORTED;
  }
  SG_REQUIRE(n_a >= 0 && n_b >= 0 && base_a >= 0 && base_b >= 0 && (measure == SG_NMS_IOU || measure == SG_NMS_MIN) &&
                 thr == thr && (adj == nullptr || (static_cast<int64_t>(base_a) + n_a <= n_total &&
                                                   static_cast<int64_t>(base_b) + n_b <= n_total)),
             "sg_mask_cross_links: bad arguments (n_a=%d n_b=%d base_a=%d base_b=%d n_total=%d measure=%d)", n_a, n_b,
             base_a, base_b, n_total, measure);
  if (n_a == 0 || n_b == 0) return SG_OK;
  SG_REQUIRE((n_bits == 0 || (bits_a != nullptr && bits_b != nullptr)) &&
                 (adj == nullptr || (labels_a != nullptr && labels_b != nullptr)),
             "sg_mask_cross_links: null array");
  ClArgs a;
  a.bits_a = bits_a, a.bits_b = bits_b, a.labels_a = labels_a, a.labels_b = labels_b, a.adj = adj;
  a.inter_out = inter_out, a.cnt_a_out = cnt_a_out, a.cnt_b_out = cnt_b_out, a.thr = thr;
  a.n_bits = n_bits, a.words = (n_bits + 31) / 32;
  a.n_a = n_a, a.n_b = n_b, a.base_a = base_a, a.base_b = base_b, a.n_total = n_total, a.nw = (n_total + 31) / 32;
  a.measure = measure, a.min_shared = min_shared;
  a.group_a = a.group_b = nullptr, a.symmetric = 0;
  cross_links_launch(a, 1 << 16, as_stream(stream_));
  return check_launch("sg_mask_cross_links");
}

int sg_stitch_components(const uint32_t *adj, int n_total, int32_t *comp, sg_stream_t stream_) {
  if (n_total < 0 || n_total > kStMaxInst) {
    set_error("sg_stitch_components: %d instances outside the supported range (<= %d)", n_total, kStMaxInst);
    return SG_ERR_UNSUPPORTED;
  }
  if (n_total == 0) return SG_OK;
  SG_REQUIRE(adj != nullptr && comp != nullptr, "sg_stitch_components: null array");
  components_kernel<<<1, kCcBlock, 0, as_stream(stream_)>>>(adj, n_total, (n_total + 31) / 32, comp);
  return check_launch("sg_stitch_components");
}

int sg_mask_bits_ids_count(const uint32_t *bits, int n_inst, int64_t n_bits, const uint8_t *core, int32_t *cnt,
                           int32_t *core_cnt, sg_stream_t stream_) {
  SG_REQUIRE(n_inst >= 0 && n_bits >= 0 && n_bits < (1LL << 31), "sg_mask_bits_ids_count: bad arguments (n_inst=%d n_bits=%lld)",
             n_inst, static_cast<long long>(n_bits));
  if (n_inst == 0) return SG_OK;
  SG_REQUIRE(cnt != nullptr && core_cnt != nullptr && (n_bits == 0 || bits != nullptr), "sg_mask_bits_ids_count: null array");
  ids_count_kernel<<<grid_for(n_inst, 1, 4096), kStBlock, 0, as_stream(stream_)>>>(bits, n_inst, n_bits, (n_bits + 31) / 32,
                                                                                 core, cnt, core_cnt);
  return check_launch("sg_mask_bits_ids_count");
}

int sg_mask_bits_ids_fill(const uint32_t *bits, int n_inst, int64_t n_bits, const int32_t *map, int64_t n_points,
                          const int64_t *row_off, const int32_t *row_key, int32_t *ids, uint32_t *keys,
                          int64_t capacity, int32_t *meta, sg_stream_t stream_) {
  SG_REQUIRE(n_inst >= 0 && n_bits >= 0 && n_bits < (1LL << 31) && n_points >= 0 && n_points < (1LL << 31) &&
                 capacity >= 0 && meta != nullptr,
             "sg_mask_bits_ids_fill: bad arguments (n_inst=%d n_bits=%lld)", n_inst, static_cast<long long>(n_bits));
  if (n_inst == 0 || n_bits == 0) return SG_OK;
  SG_REQUIRE(bits != nullptr && map != nullptr && row_off != nullptr && row_key != nullptr &&
                 (capacity == 0 || (ids != nullptr && keys != nullptr)),
             "sg_mask_bits_ids_fill: null array");
  ids_fill_kernel<<<grid_for(n_inst, 1, 4096), kStBlock, 0, as_stream(stream_)>>>(
      bits, n_inst, n_bits, (n_bits + 31) / 32, map, n_points, row_off, row_key, ids, keys, capacity, meta);
  return check_launch("sg_mask_bits_ids_fill");
}

size_t sg_stitch_union_workspace_bytes(int64_t total, int n_obj, int64_t n_points) {
  return un_in_range(total, n_obj, n_points) ? un_bytes(total) : 0;
}

int sg_stitch_union_count(const int32_t *ids, const uint32_t *keys, int64_t total, int n_obj, int64_t n_points,
                          int64_t *bounds, void *ws, size_t ws_bytes, sg_stream_t stream_) {
  if (!un_in_range(total, n_obj, n_points)) {
    set_error("sg_stitch_union_count: %lld ids, %d objects, %lld points outside the supported range (< 2^31, <= %d, "
              "< 2^31)", static_cast<long long>(total), n_obj, static_cast<long long>(n_points), kStMaxInst);
    return SG_ERR_UNSUPPORTED;
  }
  SG_REQUIRE(bounds != nullptr && (total == 0 || (ids != nullptr && keys != nullptr)), "sg_stitch_union_count: null array");
  UnWs m;
  if (!un_carve(ws, ws_bytes, total, &m)) {
    set_error("sg_stitch_union_count: workspace too small");
    return SG_ERR_WORKSPACE;
  }
  hipStream_t stream = as_stream(stream_);
  UnArgs u;
  u.k = m.keys, u.v = m.ids, u.total = total, u.n_obj = n_obj;
  if (total > 0) {
    // by id, then (stable) by object: ids ascending inside an object.  Both sorts take an even number of 8-bit
    // passes, which leaves the result in the arrays they were given (checked): the fill pass finds it there.
    un_copy_kernel<<<grid_for(total, kStBlock, 4096), kStBlock, 0, stream>>>(ids, keys, total, n_obj, n_points, m.ids, m.keys);
    uint32_t *k1;
    int32_t *v1;
    int rc = radix_sort_pairs(reinterpret_cast<uint32_t *>(m.ids), reinterpret_cast<int32_t *>(m.keys), total,
                              bit_length(n_points) > 16 ? 32 : 16, m.sort, m.sort_bytes, stream, &k1, &v1);
    if (rc != SG_OK) return rc;
    SG_REQUIRE(reinterpret_cast<int32_t *>(k1) == m.ids,
               "sg_stitch_union_count: the sort left its result outside the arrays it was given");
    uint32_t *k2;
    int32_t *v2;
    rc = radix_sort_pairs(m.keys, m.ids, total, 16, m.sort, m.sort_bytes, stream, &k2, &v2);
    if (rc != SG_OK) return rc;
    SG_REQUIRE(k2 == m.keys && v2 == m.ids,
               "sg_stitch_union_count: the sort left its result outside the arrays it was given");
  }
  int32_t *ridx = m.ridx;
  const int rc = exclusive_scan([u] __device__(int64_t e) { return un_is_start(u, e); },
                                [ridx] __device__(int64_t e, int v) { ridx[e] = v; }, total, m.total_runs, m.scan,
                                m.scan_bytes, stream);
  if (rc != SG_OK) return rc;
  un_bounds_kernel<<<grid_for(n_obj + 1, kStBlock, 64), kStBlock, 0, stream>>>(u, m.ridx, m.total_runs, bounds);
  return check_launch("sg_stitch_union_count");
}

int sg_stitch_union_fill(int64_t total, int n_obj, int64_t n_points, const void *ws, size_t ws_bytes, int32_t *starts,
                         int32_t *ends, int64_t capacity, sg_stream_t stream_) {
  if (!un_in_range(total, n_obj, n_points)) {
    set_error("sg_stitch_union_fill: outside the supported range");
    return SG_ERR_UNSUPPORTED;
  }
  SG_REQUIRE(capacity >= 0 && (capacity == 0 || (starts != nullptr && ends != nullptr)), "sg_stitch_union_fill: bad arguments");
  UnWs m;
  if (!un_carve(const_cast<void *>(ws), ws_bytes, total, &m)) {
    set_error("sg_stitch_union_fill: workspace too small");
    return SG_ERR_WORKSPACE;
  }
  if (total == 0 || capacity == 0) return SG_OK;
  hipStream_t stream = as_stream(stream_);
  UnArgs u;
  u.k = m.keys, u.v = m.ids, u.total = total, u.n_obj = n_obj;
  un_fill_kernel<<<grid_for(total, kStBlock, 4096), kStBlock, 0, stream>>>(u, m.ridx, starts, ends, capacity);
  return check_launch("sg_stitch_union_fill");
}

}  // extern "C"
