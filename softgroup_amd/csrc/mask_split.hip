// mask_split.hip -- instance masks cut into their spatially connected components (sg_mask_split_count / _fill).
//
// The reference has no counterpart: its get_instances returns every (proposal, class) pair whose mask passes the
// score and size cuts, whatever its geometry -- a chair plus stray points on the wall behind it, or two chairs the
// grouping welded together.  This stage is new, opt-in (test_cfg.split) and runs on bit rows, the layout of
// sg_mask_nms.  The rules are stated in include/softgroup_hip.h.
//
// A NODE is a (mask, point) pair; its id is its position in (mask, point) order, so inside one mask ids ascend with
// the point index and the smallest id of a component is its smallest point.  The count pass:
//   scan      exclusive prefix of the populations of all (row, word)s: id of pair (k, q) = prefix[k][q / 32] +
//             popcount of the bits below q in its word.  One read-back of the total P sizes everything below.
//   expand    one thread per word writes point and mask of its pairs and decides the validity flag -- a kernel of
//             its own, before any table is touched.
//   grid      hashed cells of `radius`, keyed by (mask, cell): a slot is claimed by the first pair that gets there
//             (atomicCAS on `owner`, the table of resample.hip), pairs are counted per slot, the counts scanned and
//             the pairs laid out cell after cell as (x, y, z, id).  Which pair owns a slot and the order inside a
//             cell depend on the order of arrival; nothing that is written out does.
//   edges     one thread per pair walks the cells its neighbours can lie in (3 per axis; 4 where the pair sits
//             within rounding of a cell face) and unites itself with every pair of LOWER id of its mask within the
//             radius.  Union-find with parent[i] <= i: find walks strictly descending ids, a root is hooked under a
//             smaller root by atomicCAS, a lost race re-finds from the value read.  Nobody waits for anybody.
//   flatten   every pair's root into an array of its own (path halving may still rewrite `parent`), sizes by
//             integer atomicAdd on the root; 'largest' by one 64-bit atomicMax per mask on (size << 32) | ~root.
//   number    survivors are numbered by a scan over the roots in id order = ascending (mask, smallest point).
// The fill pass zeroes the output rows and ORs every surviving pair's bit into its row.
//
// Bounds that do not depend on the data: a probe loop ends after `cap` probes, a find after P + 1 steps (ids
// descend strictly), a union after 2 P + 2 rounds (the sum of its two ids descends strictly), a cell walk after 4
// cells per axis; a bound that is hit sets SG_SPLIT_FLAG_INTERNAL and the thread moves on.  Every index read from
// memory is range-checked before it addresses anything.
#include "common.h"
#include "scan.h"
#include "union_find.h"

namespace sg {

constexpr int kMsBlock = 256;
constexpr int kMsMaxInst = 16384;
constexpr double kMsCellLimit = 2147483648.0;             // |cell| < 2^31
// Two pairs within the radius differ by at most 1 + 2^-50 (1 + |y|) in y = fl(x / radius) (the roundings of the
// difference, the squares, the sum and the two quotients); the walk covers floor(y - 1 - g) .. floor(y + 1 + g)
// with g = 2^-40 max(1, |y|) <= 2^-9: three cells, four next to a face.
constexpr double kMsGuard = 1.0 / 1099511627776.0;
constexpr int kMsHdrTotal = 0, kMsHdrOut = 1;             // int64 words of the workspace header

// cell of a point; false when a coordinate is not finite or a cell reaches 2^31 (NaN / inf fail the comparison)
__device__ __forceinline__ bool ms_cell(const float *__restrict__ p, double radius, int32_t c[3]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double f = floor(static_cast<double>(p[k]) / radius);
    const bool in = fabs(f) < kMsCellLimit;
    ok &= in;
    c[k] = in ? static_cast<int32_t>(f) : 0;
  }
  return ok;
}

__device__ __forceinline__ uint64_t ms_hash(int32_t k, int32_t cx, int32_t cy, int32_t cz) {
  const uint64_t a = (static_cast<uint64_t>(static_cast<uint32_t>(cx)) << 32) | static_cast<uint32_t>(cy);
  const uint64_t b = (static_cast<uint64_t>(static_cast<uint32_t>(k)) << 32) | static_cast<uint32_t>(cz);
  return mix64(a ^ mix64(b + 0x9e3779b97f4a7c15ULL));
}

inline int64_t ms_table_cap(int64_t n) {
  int64_t cap = 64;
  while (cap < 2 * n) cap <<= 1;
  return cap;
}

// ---- workspace ---------------------------------------------------------------------------------------------------
struct MsWs {
  int64_t P, cap, nw;
  int64_t *hdr;                    // [32]   kMsHdrTotal, kMsHdrOut
  int32_t *wpre;                   // [n * words + 1]  pairs before (row, word); the total behind the last
  void *scan_ws;
  size_t scan_bytes;
  unsigned long long *best;        // [n]    'largest': (size << 32) | ~root of the mask's winner
  int32_t *pt, *mk;                // [P]    point and mask of a pair
  int32_t *parent;                 // [P]    union-find, parent[i] <= i
  int32_t *size;                   // [P]    at the roots
  int32_t *outidx;                 // [P]    at the roots: output row, -1 = dropped
  uint32_t *slot_of;               // [P]    table slot of the pair's cell ...
  int32_t *root;                   //        ... and, once the grid is done with it, the pair's root
  int32_t *rank_of;                // [P]    position inside the cell, in order of arrival
  float4 *sorted;                  // [P]    (x, y, z, bits of id), cell after cell
  int32_t *owner, *count, *start;  // [cap]
  int4 *key;                       // [cap]  (cx, cy, cz, mask) of the slots in use
};

// the layout for P pairs -> bytes; with a base address the pointers too
static size_t ms_layout(int n, int64_t n_points, int64_t P, void *base, MsWs *w) {
  const size_t words = static_cast<size_t>((n_points + 31) / 32), nw = static_cast<size_t>(n) * words;
  const size_t pp = static_cast<size_t>(P > 0 ? P : 1), cap = static_cast<size_t>(ms_table_cap(P));
  size_t scan_n = nw > cap ? nw : cap;
  scan_n = scan_n > pp ? scan_n : pp;
  const size_t scan_bytes = scan_workspace_bytes(static_cast<int64_t>(scan_n));
  size_t off = 0;
  char *b = static_cast<char *>(base);
  auto take = [&](size_t bytes) {
    char *r = b == nullptr ? nullptr : b + off;
    off += align_up(bytes);
    return r;
  };
  char *hdr = take(32 * 8), *wpre = take((nw + 1) * 4), *scan = take(scan_bytes);
  char *best = take(static_cast<size_t>(n > 0 ? n : 1) * 8);
  char *pt = take(pp * 4), *mk = take(pp * 4), *parent = take(pp * 4), *size = take(pp * 4), *outidx = take(pp * 4);
  char *slot_of = take(pp * 4), *rank_of = take(pp * 4), *sorted = take(pp * 16);
  char *owner = take(cap * 4), *count = take(cap * 4), *start = take(cap * 4), *key = take(cap * 16);
  if (w != nullptr) {
    w->P = P, w->cap = static_cast<int64_t>(cap), w->nw = static_cast<int64_t>(nw);
    w->hdr = reinterpret_cast<int64_t *>(hdr), w->wpre = reinterpret_cast<int32_t *>(wpre);
    w->scan_ws = scan, w->scan_bytes = scan_bytes;
    w->best = reinterpret_cast<unsigned long long *>(best);
    w->pt = reinterpret_cast<int32_t *>(pt), w->mk = reinterpret_cast<int32_t *>(mk);
    w->parent = reinterpret_cast<int32_t *>(parent), w->size = reinterpret_cast<int32_t *>(size);
    w->outidx = reinterpret_cast<int32_t *>(outidx), w->slot_of = reinterpret_cast<uint32_t *>(slot_of);
    w->root = reinterpret_cast<int32_t *>(slot_of), w->rank_of = reinterpret_cast<int32_t *>(rank_of);
    w->sorted = reinterpret_cast<float4 *>(sorted);
    w->owner = reinterpret_cast<int32_t *>(owner), w->count = reinterpret_cast<int32_t *>(count);
    w->start = reinterpret_cast<int32_t *>(start), w->key = reinterpret_cast<int4 *>(key);
  }
  return off + 256;
}

// ---- ids ---------------------------------------------------------------------------------------------------------
struct MsPopIn {
  const uint32_t *bits;
  int64_t words;
  uint32_t tail_mask;              // of the last word of a row
  __device__ int operator()(int64_t t) const {
    uint32_t x = bits[t];
    if (t % words == words - 1) x &= tail_mask;
    return __popc(x);
  }
};
struct MsStoreOut {
  int32_t *out;
  __device__ void operator()(int64_t i, int v) const { out[i] = v; }
};

// One workgroup: the total in 64 bits from the rows' populations (each < 2^31, so the 32-bit prefix gives them
// exactly even where it has wrapped).
__global__ void __launch_bounds__(kMsBlock) ms_total_kernel(const int32_t *__restrict__ wpre, int n, int64_t words,
                                                           int64_t *__restrict__ hdr, int32_t *__restrict__ meta) {
  __shared__ long long part[kMsBlock];
  long long s = 0;
  for (int k = threadIdx.x; k < n; k += kMsBlock)
    s += static_cast<uint32_t>(wpre[(k + 1) * words]) - static_cast<uint32_t>(wpre[k * words]);
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = kMsBlock / 2; o > 0; o >>= 1) {
    if (static_cast<int>(threadIdx.x) < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    hdr[kMsHdrTotal] = part[0];
    hdr[kMsHdrOut] = 0;
    meta[2] = part[0] > INT32_MAX ? INT32_MAX : static_cast<int32_t>(part[0]);
  }
}

struct MsArgs {
  const float *xyz;
  const uint32_t *bits;
  int n, min_npoint, mode;
  int64_t n_points, words;
  uint32_t tail_mask;
  double radius, r2;
  int32_t *meta;                   // [0] outputs, [1] flags, [2] pairs, [3] components
  MsWs w;
};

// One thread per (row, word): point and mask of its pairs, every pair its own root, and the validity flag.
__global__ void __launch_bounds__(kMsBlock) ms_expand_kernel(MsArgs a) {
  int bad = 0;
  for (int64_t t = blockIdx.x * static_cast<int64_t>(kMsBlock) + threadIdx.x; t < a.w.nw;
       t += static_cast<int64_t>(gridDim.x) * kMsBlock) {
    const int64_t k = t / a.words, wq = t - k * a.words;
    uint32_t x = a.bits[t];
    if (wq == a.words - 1) x &= a.tail_mask;
    int64_t id = a.w.wpre[t];
    for (; x; x &= x - 1, ++id) {
      if (id < 0 || id >= a.w.P) {                               // (the prefix and the bits disagree: never)
        bad |= SG_SPLIT_FLAG_INTERNAL;
        break;
      }
      const int64_t q = wq * 32 + (__ffs(x) - 1);
      a.w.pt[id] = static_cast<int32_t>(q);
      a.w.mk[id] = static_cast<int32_t>(k);
      a.w.parent[id] = static_cast<int32_t>(id);
      a.w.size[id] = 0;
      const float *p = a.xyz + 3 * q;
      int32_t c[3];
      if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])))
        bad |= SG_SPLIT_FLAG_NOT_FINITE;
      else if (!ms_cell(p, a.radius, c))
        bad |= SG_SPLIT_FLAG_CELL_RANGE;
    }
  }
  if (bad) atomicOr(&a.meta[1], bad);
}

// ---- the grid ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kMsBlock) ms_insert_kernel(MsArgs a) {
  if (a.meta[1] != 0) return;                                    // invalid input: no table is touched
  const uint64_t mask = static_cast<uint64_t>(a.w.cap - 1);
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kMsBlock) + threadIdx.x; i < a.w.P;
       i += static_cast<int64_t>(gridDim.x) * kMsBlock) {
    const int32_t q = a.w.pt[i], k = a.w.mk[i];
    int64_t slot = -1;
    int32_t c[3];
    if (static_cast<uint32_t>(q) < static_cast<uint64_t>(a.n_points) && ms_cell(a.xyz + 3 * static_cast<int64_t>(q),
                                                                                a.radius, c)) {
      uint64_t s = ms_hash(k, c[0], c[1], c[2]) & mask;
      for (int64_t probe = 0; probe < a.w.cap; ++probe) {
        const int32_t o = atomicCAS(&a.w.owner[s], -1, static_cast<int32_t>(i));
        if (o == -1 || o == i) {
          slot = static_cast<int64_t>(s);
          break;
        }
        if (o < 0 || o >= a.w.P) break;
        const int32_t oq = a.w.pt[o];
        int32_t oc[3];
        if (a.w.mk[o] == k && static_cast<uint32_t>(oq) < static_cast<uint64_t>(a.n_points)) {
          ms_cell(a.xyz + 3 * static_cast<int64_t>(oq), a.radius, oc);
          if (oc[0] == c[0] && oc[1] == c[1] && oc[2] == c[2]) {
            slot = static_cast<int64_t>(s);
            break;
          }
        }
        s = (s + 1) & mask;
      }
    }
    a.w.slot_of[i] = slot < 0 ? 0xFFFFFFFFu : static_cast<uint32_t>(slot);
    a.w.rank_of[i] = slot < 0 ? 0 : atomicAdd(&a.w.count[slot], 1);
    if (slot < 0) atomicOr(&a.meta[1], SG_SPLIT_FLAG_INTERNAL);   // (cap >= 2 P: never)
  }
}

struct MsCountIn {
  const int32_t *count;
  __device__ int operator()(int64_t s) const { return count[s]; }
};

__global__ void __launch_bounds__(kMsBlock) ms_key_kernel(MsArgs a) {
  if (a.meta[1] != 0) return;
  for (int64_t s = blockIdx.x * static_cast<int64_t>(kMsBlock) + threadIdx.x; s < a.w.cap;
       s += static_cast<int64_t>(gridDim.x) * kMsBlock) {
    const int32_t o = a.w.owner[s];
    int32_t c[3] = {0, 0, 0}, k = -1;
    if (o >= 0 && o < a.w.P) {
      const int32_t q = a.w.pt[o];
      if (static_cast<uint32_t>(q) < static_cast<uint64_t>(a.n_points)) {
        ms_cell(a.xyz + 3 * static_cast<int64_t>(q), a.radius, c);
        k = a.w.mk[o];
      }
    }
    a.w.key[s] = make_int4(c[0], c[1], c[2], k);
  }
}

__global__ void __launch_bounds__(kMsBlock) ms_scatter_kernel(MsArgs a) {
  if (a.meta[1] != 0) return;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kMsBlock) + threadIdx.x; i < a.w.P;
       i += static_cast<int64_t>(gridDim.x) * kMsBlock) {
    const uint32_t s = a.w.slot_of[i];
    const int32_t q = a.w.pt[i];
    if (static_cast<int64_t>(s) >= a.w.cap || static_cast<uint32_t>(q) >= static_cast<uint64_t>(a.n_points)) continue;
    const int64_t pos = static_cast<int64_t>(a.w.start[s]) + a.w.rank_of[i];
    if (pos < 0 || pos >= a.w.P) continue;
    const float *p = a.xyz + 3 * static_cast<int64_t>(q);
    a.w.sorted[pos] = make_float4(p[0], p[1], p[2], __int_as_float(static_cast<int32_t>(i)));
  }
}

// ---- union-find (union_find.h) -----------------------------------------------------------------------------------
// One thread per pair: the pairs of lower id of its mask within the radius.
__global__ void __launch_bounds__(kMsBlock) ms_edges_kernel(MsArgs a) {
  if (a.meta[1] != 0) return;
  const uint64_t mask = static_cast<uint64_t>(a.w.cap - 1);
  bool fine = true;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kMsBlock) + threadIdx.x; i < a.w.P;
       i += static_cast<int64_t>(gridDim.x) * kMsBlock) {
    const int32_t q = a.w.pt[i], k = a.w.mk[i];
    if (static_cast<uint32_t>(q) >= static_cast<uint64_t>(a.n_points)) continue;
    const float *p = a.xyz + 3 * static_cast<int64_t>(q);
    const double px = p[0], py = p[1], pz = p[2];
    int64_t lo[3], hi[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double y = static_cast<double>(p[d]) / a.radius;
      const double g = kMsGuard * fmax(1.0, fabs(y));
      const double l = fmax(floor(y - 1.0 - g), -2147483647.0), h = fmin(floor(y + 1.0 + g), 2147483647.0);
      lo[d] = static_cast<int64_t>(l);
      hi[d] = static_cast<int64_t>(h);
      if (hi[d] > lo[d] + 3) hi[d] = lo[d] + 3;                  // (three cells, four next to a face: never more)
    }
    for (int64_t cz = lo[2]; cz <= hi[2]; ++cz)
      for (int64_t cy = lo[1]; cy <= hi[1]; ++cy)
        for (int64_t cx = lo[0]; cx <= hi[0]; ++cx) {
          const int32_t kx = static_cast<int32_t>(cx), ky = static_cast<int32_t>(cy), kz = static_cast<int32_t>(cz);
          uint64_t s = ms_hash(k, kx, ky, kz) & mask;
          for (int64_t probe = 0; probe < a.w.cap; ++probe) {
            const int32_t cnt = a.w.count[s];
            if (cnt <= 0) break;                                 // a free slot ends the chain
            const int4 key = a.w.key[s];
            if (key.x == kx && key.y == ky && key.z == kz && key.w == k) {
              const int64_t st = a.w.start[s];
              if (st >= 0 && st + cnt <= a.w.P) {
                for (int64_t t = st; t < st + cnt; ++t) {
                  const float4 v = a.w.sorted[t];
                  const int32_t j = __float_as_int(v.w);
                  if (j < 0 || j >= i) continue;
                  const double dx = px - static_cast<double>(v.x), dy = py - static_cast<double>(v.y),
                               dz = pz - static_cast<double>(v.z);
                  if ((dx * dx + dy * dy) + dz * dz <= a.r2)
                    fine &= uf_unite(a.w.parent, static_cast<int32_t>(i), j, a.w.P);
                }
              }
              break;
            }
            s = (s + 1) & mask;
          }
        }
  }
  if (!fine) atomicOr(&a.meta[1], SG_SPLIT_FLAG_INTERNAL);
}

// every pair's root, sizes at the roots, the number of components
__global__ void __launch_bounds__(kMsBlock) ms_flatten_kernel(MsArgs a) {
  if (a.meta[1] != 0) return;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kMsBlock) + threadIdx.x; i < a.w.P;
       i += static_cast<int64_t>(gridDim.x) * kMsBlock) {
    const int32_t r = uf_find(a.w.parent, static_cast<int32_t>(i), a.w.P);
    a.w.root[i] = r;
    if (r < 0) {
      atomicOr(&a.meta[1], SG_SPLIT_FLAG_INTERNAL);
      continue;
    }
    atomicAdd(&a.w.size[r], 1);
    if (r == i) atomicAdd(&a.meta[3], 1);
  }
}

__device__ __forceinline__ unsigned long long ms_rank_key(int32_t size, int32_t root) {
  return (static_cast<unsigned long long>(static_cast<uint32_t>(size)) << 32) | (~static_cast<uint32_t>(root));
}

// 'largest': the greatest size per mask, the smaller root among equal sizes
__global__ void __launch_bounds__(kMsBlock) ms_best_kernel(MsArgs a) {
  if (a.meta[1] != 0) return;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kMsBlock) + threadIdx.x; i < a.w.P;
       i += static_cast<int64_t>(gridDim.x) * kMsBlock) {
    const int32_t k = a.w.mk[i];
    if (a.w.root[i] != i || static_cast<uint32_t>(k) >= static_cast<uint32_t>(a.n)) continue;
    atomicMax(&a.w.best[k], ms_rank_key(a.w.size[i], static_cast<int32_t>(i)));
  }
}

struct MsKeepIn {
  const int32_t *root, *size, *mk, *flags;
  const unsigned long long *best;
  int n, min_npoint, mode;
  __device__ int operator()(int64_t i) const {
    if (*flags != 0 || root[i] != i) return 0;
    const int32_t s = size[i], k = mk[i];
    if (s < min_npoint || static_cast<uint32_t>(k) >= static_cast<uint32_t>(n)) return 0;
    if (mode == SG_SPLIT_LARGEST) return best[k] == ms_rank_key(s, static_cast<int32_t>(i)) ? 1 : 0;
    return 1;
  }
};
struct MsKeepOut {
  MsKeepIn in;
  int32_t *outidx;
  __device__ void operator()(int64_t i, int v) const { outidx[i] = in(i) ? v : -1; }
};

// n_out arrives as the scan's total in the low half of hdr[kMsHdrOut] (the high half is zero)
__global__ void ms_finish_kernel(int64_t *__restrict__ hdr, int32_t *__restrict__ meta) {
  const int32_t n_out = meta[1] != 0 ? 0 : reinterpret_cast<const int32_t *>(hdr + kMsHdrOut)[0];
  meta[0] = n_out;
  if (n_out > kMsMaxInst) meta[1] |= SG_SPLIT_FLAG_TOO_MANY;
  hdr[kMsHdrOut] = n_out > kMsMaxInst ? 0 : n_out;
}

// ---- fill --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kMsBlock) ms_zero_kernel(const int64_t *__restrict__ hdr, int64_t words,
                                                          int64_t capacity, uint32_t *__restrict__ out_bits) {
  int64_t rows = hdr[kMsHdrOut];
  rows = rows < capacity ? rows : capacity;
  if (rows < 0 || rows > kMsMaxInst) return;
  for (int64_t t = blockIdx.x * static_cast<int64_t>(kMsBlock) + threadIdx.x; t < rows * words;
       t += static_cast<int64_t>(gridDim.x) * kMsBlock)
    out_bits[t] = 0u;
}

__global__ void __launch_bounds__(kMsBlock) ms_emit_kernel(MsWs w, int n, int64_t n_points, int64_t words,
                                                          int64_t capacity, uint32_t *__restrict__ out_bits,
                                                          int32_t *__restrict__ source, int32_t *__restrict__ npoint) {
  int64_t rows = w.hdr[kMsHdrOut];
  rows = rows < capacity ? rows : capacity;
  if (rows <= 0 || rows > kMsMaxInst) return;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kMsBlock) + threadIdx.x; i < w.P;
       i += static_cast<int64_t>(gridDim.x) * kMsBlock) {
    const int32_t r = w.root[i];
    if (r < 0 || r >= w.P) continue;
    const int32_t o = w.outidx[r];
    const int32_t q = w.pt[i];
    if (o < 0 || o >= rows || static_cast<uint32_t>(q) >= static_cast<uint64_t>(n_points)) continue;
    atomicOr(&out_bits[o * words + (q >> 5)], 1u << (q & 31));
    if (r == i) {
      source[o] = w.mk[i];
      npoint[o] = w.size[i];
    }
  }
}

}  // namespace sg

using namespace sg;

extern "C" {

static bool split_in_range(int n_inst, int64_t n_points, int64_t n_pairs) {
  return n_inst >= 0 && n_inst <= kMsMaxInst && n_points >= 0 && n_points < (1LL << 31) && n_pairs >= 0 &&
         n_pairs < (1LL << 31);
}

size_t sg_mask_split_workspace_bytes(int n_inst, int64_t n_points, int64_t n_pairs) {
  if (!split_in_range(n_inst, n_points, n_pairs)) return 0;
  return ms_layout(n_inst, n_points, n_pairs, nullptr, nullptr);
}

int sg_mask_split_count(const float *xyz, const uint32_t *bits, int n_inst, int64_t n_points, double radius,
                        int min_npoint, int mode, int32_t *meta, void *ws, size_t ws_bytes, sg_stream_t stream_) {
  if (!split_in_range(n_inst, n_points, 0)) {
    set_error("sg_mask_split_count: n_inst %d, n_points %lld outside the supported range (n_inst <= %d, "
              "n_points < 2^31)", n_inst, static_cast<long long>(n_points), kMsMaxInst);
    return SG_ERR_UNSUPPORTED;
  }
  SG_REQUIRE(meta != nullptr && radius > 0.0 && radius * radius < __builtin_inf() && min_npoint >= 1 &&
                 (mode == SG_SPLIT_ALL || mode == SG_SPLIT_LARGEST),
             "sg_mask_split_count: bad arguments (radius %g, min_npoint %d, mode %d)", radius, min_npoint, mode);
  hipStream_t stream = as_stream(stream_);
  hipMemsetAsync(meta, 0, 4 * sizeof(int32_t), stream);
  if (n_inst == 0 || n_points == 0) return check_launch("sg_mask_split_count");
  SG_REQUIRE(xyz != nullptr && bits != nullptr, "sg_mask_split_count: null array");
  if (ws == nullptr || ws_bytes < ms_layout(n_inst, n_points, 0, nullptr, nullptr)) {
    set_error("sg_mask_split_count: workspace too small (%zu bytes, %zu needed before the pairs are counted)",
              ws_bytes, ms_layout(n_inst, n_points, 0, nullptr, nullptr));
    return SG_ERR_WORKSPACE;
  }
  int32_t *host = pinned_words();
  SG_REQUIRE(host != nullptr, "sg_mask_split_count: no pinned host words");

  MsArgs a;
  a.xyz = xyz, a.bits = bits, a.n = n_inst, a.min_npoint = min_npoint, a.mode = mode;
  a.n_points = n_points, a.words = (n_points + 31) / 32;
  a.tail_mask = (n_points & 31) ? (1u << (n_points & 31)) - 1u : 0xFFFFFFFFu;
  a.radius = radius, a.r2 = radius * radius, a.meta = meta;
  ms_layout(n_inst, n_points, 0, ws, &a.w);            // (header, prefix and scan space do not move with P)

  // ---- ids: the prefix over all words, the total in 64 bits, one read-back
  int rc = exclusive_scan(MsPopIn{bits, a.words, a.tail_mask}, MsStoreOut{a.w.wpre}, a.w.nw, a.w.wpre + a.w.nw,
                          a.w.scan_ws, a.w.scan_bytes, stream);
  if (rc != SG_OK) return rc;
  ms_total_kernel<<<1, kMsBlock, 0, stream>>>(a.w.wpre, n_inst, a.words, a.w.hdr, meta);
  rc = check_launch("sg_mask_split_count");
  if (rc != SG_OK) return rc;
  int64_t *h = reinterpret_cast<int64_t *>(host);
  if (hipMemcpyAsync(h, a.w.hdr, 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess) {
    set_error("sg_mask_split_count: read-back failed");
    return SG_ERR_LAUNCH;
  }
  const int64_t P = h[0];
  if (P < 0 || P >= (1LL << 31)) {
    set_error("sg_mask_split_count: %lld mask points in all, the supported range ends below 2^31",
              static_cast<long long>(P));
    return SG_ERR_UNSUPPORTED;
  }
  if (P == 0) return SG_OK;
  const size_t need = ms_layout(n_inst, n_points, P, nullptr, nullptr);
  if (ws_bytes < need) {
    set_error("sg_mask_split_count: workspace too small (%zu bytes) for %lld mask points: %zu needed", ws_bytes,
              static_cast<long long>(P), need);
    return SG_ERR_WORKSPACE;                           // (meta[2] holds P; nothing beyond the prefix was written)
  }
  ms_layout(n_inst, n_points, P, ws, &a.w);

  // ---- pairs, validity, the grid
  FillList f;
  f.add(a.w.owner, static_cast<size_t>(a.w.cap) * 4, 0xFF);
  f.add(a.w.count, static_cast<size_t>(a.w.cap) * 4, 0);
  f.add(a.w.best, static_cast<size_t>(n_inst) * 8, 0);
  fill_many(f, stream);
  ms_expand_kernel<<<grid_for(a.w.nw, kMsBlock), kMsBlock, 0, stream>>>(a);
  const int gp = grid_for(P, kMsBlock, 8192), gc = grid_for(a.w.cap, kMsBlock, 8192);
  ms_insert_kernel<<<gp, kMsBlock, 0, stream>>>(a);
  rc = exclusive_scan(MsCountIn{a.w.count}, MsStoreOut{a.w.start}, a.w.cap, nullptr, a.w.scan_ws, a.w.scan_bytes,
                      stream);
  if (rc != SG_OK) return rc;
  ms_key_kernel<<<gc, kMsBlock, 0, stream>>>(a);
  ms_scatter_kernel<<<gp, kMsBlock, 0, stream>>>(a);
  // ---- components, sizes, selection, numbering
  ms_edges_kernel<<<gp, kMsBlock, 0, stream>>>(a);
  ms_flatten_kernel<<<gp, kMsBlock, 0, stream>>>(a);
  if (mode == SG_SPLIT_LARGEST) ms_best_kernel<<<gp, kMsBlock, 0, stream>>>(a);
  const MsKeepIn keep{a.w.root, a.w.size, a.w.mk, meta + 1, a.w.best, n_inst, min_npoint, mode};
  rc = exclusive_scan(keep, MsKeepOut{keep, a.w.outidx}, P, reinterpret_cast<int32_t *>(a.w.hdr + kMsHdrOut),
                      a.w.scan_ws, a.w.scan_bytes, stream);
  if (rc != SG_OK) return rc;
  ms_finish_kernel<<<1, 1, 0, stream>>>(a.w.hdr, meta);
  return check_launch("sg_mask_split_count");
}

int sg_mask_split_fill(int n_inst, int64_t n_points, int64_t n_pairs, const void *ws, size_t ws_bytes,
                       int64_t capacity, uint32_t *out_bits, int32_t *source, int32_t *npoint, sg_stream_t stream_) {
  if (!split_in_range(n_inst, n_points, n_pairs)) {
    set_error("sg_mask_split_fill: n_inst %d, n_points %lld, %lld mask points outside the supported range", n_inst,
              static_cast<long long>(n_points), static_cast<long long>(n_pairs));
    return SG_ERR_UNSUPPORTED;
  }
  SG_REQUIRE(capacity >= 0, "sg_mask_split_fill: negative capacity");
  if (n_pairs == 0 || capacity == 0 || n_inst == 0) return SG_OK;      // no mask point: no output
  SG_REQUIRE(out_bits != nullptr && source != nullptr && npoint != nullptr, "sg_mask_split_fill: null array");
  if (ws == nullptr || ws_bytes < ms_layout(n_inst, n_points, n_pairs, nullptr, nullptr)) {
    set_error("sg_mask_split_fill: workspace too small");
    return SG_ERR_WORKSPACE;
  }
  hipStream_t stream = as_stream(stream_);
  MsWs w;
  ms_layout(n_inst, n_points, n_pairs, const_cast<void *>(ws), &w);
  const int64_t words = (n_points + 31) / 32;
  const int64_t cap_rows = capacity < kMsMaxInst ? capacity : kMsMaxInst;
  ms_zero_kernel<<<grid_for(cap_rows * words, kMsBlock, 8192), kMsBlock, 0, stream>>>(w.hdr, words, capacity, out_bits);
  ms_emit_kernel<<<grid_for(n_pairs, kMsBlock, 8192), kMsBlock, 0, stream>>>(w, n_inst, n_points, words, capacity,
                                                                             out_bits, source, npoint);
  return check_launch("sg_mask_split_fill");
}

}  // extern "C"
