// point_grid.h -- the hashed uniform grid over a point cloud that resample.hip (nearest source point) and
// geometry.hip (k nearest neighbours) share: cells, the hash, the table of slots and the build that lays the points
// out cell after cell.
//
// The table: open addressing, capacity a power of two >= 2 n.  A slot is claimed by the index of the first point
// that gets there (atomicCAS on `owner`); a later point compares its cell with the cell of the slot's owner,
// recomputed from the owner's coordinates -- no key has to become visible inside the kernel that inserts.  Which
// point owns a slot and the order inside a cell depend on the order of arrival, nothing that is written out does.
//
// Bounds that do not depend on the data: every probe loop ends after `cap` probes; every index read from memory is
// range-checked before it addresses anything; a kernel that touches a table first reads the validity flags the
// kernel before it left.
#pragma once
#include "common.h"
#include "scan.h"

namespace sg {

constexpr int kRsBlock = 256;
constexpr double kNnCellLimit = 1073741824.0;        // |cell| < 2^30 (the point grid: room for the shells)
// A point outside shells 0 .. R differs from the query by more than R cells along one axis.  The cell of a
// coordinate is floor(fl(x / cell)), monotone in x, so cells are intervals whose ends lie within
// |c| 2^-52 <= 2^-22 cells of the exact k * cell: its d2 is at least (R cell)^2 (1 - 2^-21).  The walk stops
// below (R cell)^2 (1 - 2^-18), strictly: nothing outside can be nearer, or as near with a lower index.
constexpr double kNnStopMargin = 1.0 - 1.0 / 262144.0;

constexpr int kFlagBadSrc = 1, kFlagBadQuery = 2, kFlagNoGrid = 4;

// cell of a point; false when a coordinate is not finite or a cell reaches `limit` (NaN / inf fail the comparison)
__device__ __forceinline__ bool cell_of(const float *__restrict__ p, double voxel, double limit, int32_t c[3]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double f = floor(static_cast<double>(p[k]) / voxel);
    const bool in = fabs(f) < limit;
    ok &= in;
    c[k] = in ? static_cast<int32_t>(f) : 0;
  }
  return ok;
}

__device__ __forceinline__ uint64_t cell_hash(int32_t cx, int32_t cy, int32_t cz) {
  const uint64_t a = (static_cast<uint64_t>(static_cast<uint32_t>(cx)) << 32) | static_cast<uint32_t>(cy);
  return mix64(a ^ mix64(static_cast<uint64_t>(static_cast<uint32_t>(cz)) + 0x9e3779b97f4a7c15ULL));
}

// slot of point i's cell, claiming a free one; -1 after `cap` probes or on an owner outside [0, n)
__device__ __forceinline__ int64_t table_insert(int32_t *__restrict__ owner, int64_t cap, const float *__restrict__ xyz,
                                               int64_t n, double voxel, double limit, int32_t i, const int32_t c[3]) {
  uint64_t s = cell_hash(c[0], c[1], c[2]) & static_cast<uint64_t>(cap - 1);
  for (int64_t probe = 0; probe < cap; ++probe) {
    const int32_t o = atomicCAS(&owner[s], -1, i);
    if (o == -1 || o == i) return static_cast<int64_t>(s);
    if (o < 0 || o >= n) return -1;
    int32_t oc[3];
    cell_of(xyz + 3 * static_cast<int64_t>(o), voxel, limit, oc);
    if (oc[0] == c[0] && oc[1] == c[1] && oc[2] == c[2]) return static_cast<int64_t>(s);
    s = (s + 1) & static_cast<uint64_t>(cap - 1);
  }
  return -1;
}

inline int64_t table_cap(int64_t n) {
  int64_t cap = 64;
  while (cap < 2 * n) cap <<= 1;
  return cap;
}

// ---- validity ------------------------------------------------------------------------------------------------
// bit_finite for a coordinate that is not finite, bit_range for a cell at or beyond `limit`
static __global__ void __launch_bounds__(kRsBlock) rs_validate_kernel(const float *__restrict__ xyz, int64_t n,
                                                                     double voxel, double limit, int bit_finite,
                                                                     int bit_range, int32_t *__restrict__ flags) {
  int bad = 0;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kRsBlock) + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kRsBlock) {
    const float *p = xyz + 3 * i;
    int32_t c[3];
    if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])))
      bad |= bit_finite;
    else if (!cell_of(p, voxel, limit, c))
      bad |= bit_range;
  }
  if (bad) atomicOr(flags, bad);
}

// ---- the grid ------------------------------------------------------------------------------------------------
struct NnGrid {
  int64_t cap;
  int32_t *owner;        // [cap]
  int32_t *count;        // [cap]  points of the slot's cell, 0 = free
  int4 *key;             // [cap]  (cx, cy, cz, start) of the slots in use
  uint32_t *slot_of;     // [n_src]
  int32_t *rank_of;      // [n_src] position inside the cell, in order of arrival
  float4 *sorted;        // [n_src] (x, y, z, bits of j), cell after cell
  void *scan_ws;
  size_t scan_bytes;
};

static size_t nn_grid_bytes(int64_t n) {
  const size_t nn = static_cast<size_t>(n > 0 ? n : 1), cap = static_cast<size_t>(table_cap(n));
  return 2 * align_up(cap * 4) + align_up(cap * 16) + 2 * align_up(nn * 4) + align_up(nn * 16) +
         align_up(scan_workspace_bytes(static_cast<int64_t>(cap))) + 256;
}

static bool nn_carve(void *ws, size_t ws_bytes, int64_t n, NnGrid *g) {
  if (ws == nullptr || ws_bytes < nn_grid_bytes(n)) return false;
  const size_t nn = static_cast<size_t>(n > 0 ? n : 1);
  Workspace a(ws, ws_bytes);
  g->cap = table_cap(n);
  g->owner = a.take<int32_t>(g->cap);
  g->count = a.take<int32_t>(g->cap);
  g->key = a.take<int4>(g->cap);
  g->slot_of = a.take<uint32_t>(nn);
  g->rank_of = a.take<int32_t>(nn);
  g->sorted = a.take<float4>(nn);
  g->scan_bytes = scan_workspace_bytes(g->cap);
  g->scan_ws = a.take<char>(g->scan_bytes);
  return g->scan_ws != nullptr;
}

static __global__ void __launch_bounds__(kRsBlock) nn_insert_kernel(const float *__restrict__ src, int64_t n,
                                                                   double cell, const int32_t *__restrict__ flags,
                                                                   NnGrid g) {
  if (*flags & (kFlagBadSrc | kFlagNoGrid)) return;               // no grid: every query takes the full scan
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kRsBlock) + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kRsBlock) {
    int32_t c[3];
    int64_t s = -1;
    if (cell_of(src + 3 * i, cell, kNnCellLimit, c))
      s = table_insert(g.owner, g.cap, src, n, cell, kNnCellLimit, static_cast<int32_t>(i), c);
    g.slot_of[i] = s < 0 ? 0xFFFFFFFFu : static_cast<uint32_t>(s);
    g.rank_of[i] = s < 0 ? 0 : atomicAdd(&g.count[s], 1);
  }
}

static __global__ void __launch_bounds__(kRsBlock) nn_key_kernel(const float *__restrict__ src, int64_t n, double cell,
                                                                const int32_t *__restrict__ flags, NnGrid g) {
  if (*flags & (kFlagBadSrc | kFlagNoGrid)) return;
  for (int64_t s = blockIdx.x * static_cast<int64_t>(kRsBlock) + threadIdx.x; s < g.cap;
       s += static_cast<int64_t>(gridDim.x) * kRsBlock) {
    const int32_t o = g.owner[s];
    int32_t c[3] = {0, 0, 0};
    if (o >= 0 && o < n) cell_of(src + 3 * static_cast<int64_t>(o), cell, kNnCellLimit, c);
    g.key[s] = make_int4(c[0], c[1], c[2], g.key[s].w);
  }
}

static __global__ void __launch_bounds__(kRsBlock) nn_scatter_kernel(const float *__restrict__ src, int64_t n,
                                                                    const int32_t *__restrict__ flags, NnGrid g) {
  if (*flags & (kFlagBadSrc | kFlagNoGrid)) return;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kRsBlock) + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kRsBlock) {
    const uint32_t s = g.slot_of[i];
    if (static_cast<int64_t>(s) >= g.cap) continue;
    const int64_t pos = static_cast<int64_t>(g.key[s].w) + g.rank_of[i];
    if (pos < 0 || pos >= n) continue;
    g.sorted[pos] = make_float4(src[3 * i], src[3 * i + 1], src[3 * i + 2], __int_as_float(static_cast<int32_t>(i)));
  }
}

struct NnCountIn {
  const int32_t *count;
  __device__ int operator()(int64_t s) const { return count[s]; }
};
struct NnStartOut {
  int4 *key;
  __device__ void operator()(int64_t s, int v) const { key[s].w = v; }
};

// The launches that fill a carved grid from `src`; `flags` (device) is zero on entry and receives kFlagBadSrc /
// kFlagNoGrid from a kernel of its own, before the kernel that inserts.  owner / count must be filled (-1 / 0) by
// the caller on the same stream.  `max_blocks` caps the grids of the point and slot kernels (grid-stride loops).
static int nn_grid_build(const float *src, int64_t n_src, double cell, const NnGrid &g, int32_t *flags, int max_blocks,
                         hipStream_t stream) {
  const int grid_n = grid_for(n_src, kRsBlock, max_blocks);
  rs_validate_kernel<<<grid_n, kRsBlock, 0, stream>>>(src, n_src, cell, kNnCellLimit, kFlagBadSrc, kFlagNoGrid, flags);
  nn_insert_kernel<<<grid_n, kRsBlock, 0, stream>>>(src, n_src, cell, flags, g);
  // the starts of the cells go straight into the fourth component of the keys; nn_key_kernel adds the cells
  const int rc = exclusive_scan(NnCountIn{g.count}, NnStartOut{g.key}, g.cap, nullptr, g.scan_ws, g.scan_bytes, stream);
  if (rc != SG_OK) return rc;
  nn_key_kernel<<<grid_for(g.cap, kRsBlock, max_blocks), kRsBlock, 0, stream>>>(src, n_src, cell, flags, g);
  nn_scatter_kernel<<<grid_n, kRsBlock, 0, stream>>>(src, n_src, flags, g);
  return SG_OK;
}

__device__ __forceinline__ double nn_d2(double qx, double qy, double qz, float sx, float sy, float sz) {
  const double dx = qx - static_cast<double>(sx), dy = qy - static_cast<double>(sy), dz = qz - static_cast<double>(sz);
  return (dx * dx + dy * dy) + dz * dz;
}

}  // namespace sg
