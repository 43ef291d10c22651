// resample.hip -- thinning a cloud before the network and carrying results back to every original point:
// voxel-grid downsample (sg_grid_downsample), exact nearest source point (sg_nearest_build / sg_nearest_query),
// bit-row masks through an index map (sg_mask_bits_gather) and bit rows -> runs (sg_mask_runs_count / _fill).
// The rules are stated in include/softgroup_hip.h; the reference has no counterpart of any of them (its
// dataset/s3dis/downsample.py draws a random sample on the host and raises for --voxel-size).
//
// Everything here is integer or IEEE double arithmetic (-ffp-contract=off), selection by integer atomics only:
// two calls on the same input give the same bytes.
//
// Bounds that do not depend on the data: every probe loop ends after `cap` probes (the table's capacity), the
// shell walk after kNnMaxShell shells; every index read from memory is range-checked before it addresses
// anything; a kernel that touches a table first reads the validity flags the kernel before it left in meta[1].
//
// The hash table (both users), its build and the validity kernel live in point_grid.h, which geometry.hip shares.
#include "point_grid.h"

namespace sg {

constexpr int kNnMaxShell = 2;                       // shells 0, 1, 2 of cells, then the full scan
constexpr double kRsCellLimit = 2147483648.0;        // |cell| < 2^31 (sg_grid_downsample)
constexpr int kFlagBadIndex = 1;

// ---- voxel-grid downsample -----------------------------------------------------------------------------------
// d2 of point p to the centre of its cell, in the order the header states
__device__ __forceinline__ double center_d2(const float *__restrict__ p, const int32_t c[3], double voxel) {
  const double dx = static_cast<double>(p[0]) - (static_cast<double>(c[0]) + 0.5) * voxel;
  const double dy = static_cast<double>(p[1]) - (static_cast<double>(c[1]) + 0.5) * voxel;
  const double dz = static_cast<double>(p[2]) - (static_cast<double>(c[2]) + 0.5) * voxel;
  return (dx * dx + dy * dy) + dz * dz;
}

struct DsArgs {
  const float *xyz;
  int64_t n, cap;
  double voxel;
  int pick;
  const int32_t *flags;            // meta + 1
  int32_t *owner;                  // [cap]  -1 = free
  uint32_t *best_idx;              // [cap]  0xFFFFFFFF = none
  unsigned long long *best_d2;     // [cap]  bit pattern of the smallest d2 (all ones = none)
  uint32_t *slot_of;               // [n]    0xFFFFFFFF = none
  int32_t *pos;                    // [n]    exclusive count of representatives below i
};

__global__ void __launch_bounds__(kRsBlock) ds_insert_kernel(DsArgs a) {
  if (*a.flags != 0) return;                                      // invalid input: no table is touched
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kRsBlock) + threadIdx.x; i < a.n;
       i += static_cast<int64_t>(gridDim.x) * kRsBlock) {
    const float *p = a.xyz + 3 * i;
    int32_t c[3];
    int64_t s = -1;
    if (cell_of(p, a.voxel, kRsCellLimit, c))
      s = table_insert(a.owner, a.cap, a.xyz, a.n, a.voxel, kRsCellLimit, static_cast<int32_t>(i), c);
    a.slot_of[i] = s < 0 ? 0xFFFFFFFFu : static_cast<uint32_t>(s);
    if (s < 0) continue;
    if (a.pick == SG_PICK_FIRST)
      atomicMin(&a.best_idx[s], static_cast<uint32_t>(i));
    else
      atomicMin(&a.best_d2[s], static_cast<unsigned long long>(__double_as_longlong(center_d2(p, c, a.voxel))));
  }
}

// CENTER: among the points that hold their voxel's smallest d2, the lowest index
__global__ void __launch_bounds__(kRsBlock) ds_select_kernel(DsArgs a) {
  if (*a.flags != 0) return;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kRsBlock) + threadIdx.x; i < a.n;
       i += static_cast<int64_t>(gridDim.x) * kRsBlock) {
    const uint32_t s = a.slot_of[i];
    if (static_cast<int64_t>(s) >= a.cap) continue;
    const float *p = a.xyz + 3 * i;
    int32_t c[3];
    cell_of(p, a.voxel, kRsCellLimit, c);
    const unsigned long long d = static_cast<unsigned long long>(__double_as_longlong(center_d2(p, c, a.voxel)));
    if (d == a.best_d2[s]) atomicMin(&a.best_idx[s], static_cast<uint32_t>(i));
  }
}

__device__ __forceinline__ int ds_is_rep(const DsArgs &a, int64_t i) {
  if (*a.flags != 0) return 0;
  const uint32_t s = a.slot_of[i];
  if (static_cast<int64_t>(s) >= a.cap) return 0;
  return a.best_idx[s] == static_cast<uint32_t>(i) ? 1 : 0;
}

__global__ void __launch_bounds__(kRsBlock) ds_emit_kernel(DsArgs a, int32_t *__restrict__ sample_ids,
                                                          int32_t *__restrict__ inverse) {
  const bool bad = *a.flags != 0;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kRsBlock) + threadIdx.x; i < a.n;
       i += static_cast<int64_t>(gridDim.x) * kRsBlock) {
    int32_t inv = -1;
    if (!bad) {
      const uint32_t s = a.slot_of[i];
      if (static_cast<int64_t>(s) < a.cap) {
        const uint32_t r = a.best_idx[s];
        if (static_cast<int64_t>(r) < a.n) {
          const int32_t q = a.pos[r];
          if (q >= 0 && q < a.n) {
            inv = q;
            if (static_cast<int64_t>(r) == i) sample_ids[q] = static_cast<int32_t>(i);
          }
        }
      }
    }
    inverse[i] = inv;
  }
}

// ---- nearest source point ------------------------------------------------------------------------------------
// (the grid, its build kernels and nn_d2: point_grid.h)
__device__ __forceinline__ void nn_write(int64_t q, double d2, int32_t j, double max_dist, int32_t *__restrict__ index,
                                        double *__restrict__ dist2) {
  if (j < 0 || (max_dist >= 0.0 && d2 > max_dist * max_dist)) {
    j = -1;
    d2 = __longlong_as_double(0x7FF0000000000000LL);
  }
  index[q] = j;
  if (dist2 != nullptr) dist2[q] = d2;
}

// One thread per query: the shells of cells around the query's cell, at most kNnMaxShell of them.  A query that
// is not decided by then (or has no cell in the grid's range) goes onto the work list of the full scan.
__global__ void __launch_bounds__(kRsBlock) nn_query_kernel(NnGrid g, int64_t n_src, double cell,
                                                           const float *__restrict__ query, int64_t n_query,
                                                           double max_dist, int32_t *__restrict__ index,
                                                           double *__restrict__ dist2, int32_t *__restrict__ meta,
                                                           int32_t *__restrict__ work) {
  const int32_t src_flags = meta[1] & (kFlagBadSrc | kFlagNoGrid);      // (set by the build; this kernel adds others)
  const bool bad_src = (src_flags & kFlagBadSrc) != 0, no_grid = src_flags != 0;
  for (int64_t q = blockIdx.x * static_cast<int64_t>(kRsBlock) + threadIdx.x; q < n_query;
       q += static_cast<int64_t>(gridDim.x) * kRsBlock) {
    const float *p = query + 3 * q;
    const bool bad_query = !(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]));
    if (bad_src || bad_query) {      // the caller's error either way: -1 at once, no scan of the sources for it
      if (bad_query) atomicOr(&meta[1], kFlagBadQuery);
      nn_write(q, 0.0, -1, max_dist, index, dist2);
      continue;
    }
    int32_t c[3];
    bool done = false;
    double best = __longlong_as_double(0x7FF0000000000000LL);
    int32_t best_j = INT32_MAX;
    if (!no_grid && cell_of(p, cell, kNnCellLimit, c)) {
      const double qx = p[0], qy = p[1], qz = p[2];
      for (int R = 0; R <= kNnMaxShell && !done; ++R) {
        for (int dz = -R; dz <= R; ++dz)
          for (int dy = -R; dy <= R; ++dy)
            for (int dx = -R; dx <= R; ++dx) {
              if (max(max(abs(dx), abs(dy)), abs(dz)) != R) continue;
              const int32_t cx = c[0] + dx, cy = c[1] + dy, cz = c[2] + dz;      // |c| < 2^30: no overflow
              uint64_t s = cell_hash(cx, cy, cz) & static_cast<uint64_t>(g.cap - 1);
              for (int64_t probe = 0; probe < g.cap; ++probe) {
                const int32_t cnt = g.count[s];
                if (cnt <= 0) break;                                           // a free slot ends the chain
                const int4 k = g.key[s];
                if (k.x == cx && k.y == cy && k.z == cz) {
                  if (k.w >= 0 && static_cast<int64_t>(k.w) + cnt <= n_src) {
                    for (int32_t t = k.w; t < k.w + cnt; ++t) {
                      const float4 v = g.sorted[t];
                      const int32_t j = __float_as_int(v.w);
                      const double d2 = nn_d2(qx, qy, qz, v.x, v.y, v.z);
                      if (j >= 0 && j < n_src && (d2 < best || (d2 == best && j < best_j))) best = d2, best_j = j;
                    }
                  }
                  break;
                }
                s = (s + 1) & static_cast<uint64_t>(g.cap - 1);
              }
            }
        const double bound = (static_cast<double>(R) * cell) * (static_cast<double>(R) * cell) * kNnStopMargin;
        done = best_j != INT32_MAX && (R == 0 ? best == 0.0 : best < bound);
      }
    }
    if (done) {
      nn_write(q, best, best_j, max_dist, index, dist2);
    } else {
      const int32_t w = atomicAdd(&meta[0], 1);
      if (w >= 0 && w < n_query) work[w] = static_cast<int32_t>(q);
    }
  }
}

// One workgroup per listed query: every source point, the same (d2, j) order.
__global__ void __launch_bounds__(kRsBlock) nn_scan_kernel(const float *__restrict__ src, int64_t n_src,
                                                          const float *__restrict__ query, int64_t n_query,
                                                          double max_dist, int32_t *__restrict__ index,
                                                          double *__restrict__ dist2, const int32_t *__restrict__ meta,
                                                          const int32_t *__restrict__ work) {
  __shared__ double s_d2[kRsBlock];
  __shared__ int32_t s_j[kRsBlock];
  const int tid = threadIdx.x;
  int64_t n_work = meta[0];
  n_work = n_work < 0 ? 0 : (n_work > n_query ? n_query : n_work);
  for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {      // (block-uniform)
    const int64_t q = work[w];
    if (q < 0 || q >= n_query) continue;
    const double qx = query[3 * q], qy = query[3 * q + 1], qz = query[3 * q + 2];
    double best = __longlong_as_double(0x7FF0000000000000LL);
    int32_t best_j = INT32_MAX;
    for (int64_t j = tid; j < n_src; j += kRsBlock) {             // ascending j per thread: < keeps the lowest
      const double d2 = nn_d2(qx, qy, qz, src[3 * j], src[3 * j + 1], src[3 * j + 2]);
      if (d2 < best) best = d2, best_j = static_cast<int32_t>(j);
    }
    s_d2[tid] = best, s_j[tid] = best_j;
    __syncthreads();
    for (int o = kRsBlock / 2; o > 0; o >>= 1) {
      if (tid < o) {
        const double d = s_d2[tid + o];
        const int32_t j = s_j[tid + o];
        if (d < s_d2[tid] || (d == s_d2[tid] && j < s_j[tid])) s_d2[tid] = d, s_j[tid] = j;
      }
      __syncthreads();
    }
    if (tid == 0) nn_write(q, s_d2[0], s_j[0] == INT32_MAX ? -1 : s_j[0], max_dist, index, dist2);
    __syncthreads();
  }
}

// ---- masks through an index map ------------------------------------------------------------------------------
// One wave per 64 consecutive output points: their indices once (coalesced), then row after row one gathered bit
// per lane and a ballot = two output words.
__global__ void __launch_bounds__(kRsBlock) mask_gather_kernel(const uint32_t *__restrict__ bits, int n_inst,
                                                              int64_t n_src, int64_t words_src,
                                                              const int32_t *__restrict__ index, int64_t n_out,
                                                              int64_t words_out, uint32_t *__restrict__ out,
                                                              int32_t *__restrict__ meta) {
  const int lane = lane_id();
  const int64_t chunks = (n_out + 63) / 64;
  const int64_t wave = blockIdx.x * static_cast<int64_t>(kRsBlock / kWave) + (threadIdx.x >> 6);
  const int64_t waves = static_cast<int64_t>(gridDim.x) * (kRsBlock / kWave);
  for (int64_t ch = wave; ch < chunks; ch += waves) {             // (wave-uniform)
    const int64_t i = ch * 64 + lane;
    int64_t j = -1;
    if (i < n_out) {
      j = index[i];
      if (j >= n_src) {
        j = -1;
        if (meta != nullptr) atomicOr(meta, kFlagBadIndex);
      }
    }
    const int64_t word = j >> 5;
    const int sh = static_cast<int>(j & 31);
    for (int k = 0; k < n_inst; ++k) {
      bool b = false;
      if (j >= 0) b = (bits[static_cast<int64_t>(k) * words_src + word] >> sh) & 1u;
      const uint64_t m = __ballot(b);
      if (lane < 2 && 2 * ch + lane < words_out)
        out[static_cast<int64_t>(k) * words_out + 2 * ch + lane] = static_cast<uint32_t>(m >> (32 * lane));
    }
  }
}

// bits of word t (column w of its row) where a run starts / ends; `open` = 1 when a run of the words before
// it is still open at the word's first bit
__device__ __forceinline__ uint32_t runs_word(const uint32_t *__restrict__ bits, int64_t t, int64_t w, int64_t words,
                                             int tail, uint32_t *open, uint32_t *ends) {
  uint32_t x = bits[t];
  if (w == words - 1 && tail) x &= (1u << tail) - 1u;
  const uint32_t prev = w > 0 ? bits[t - 1] >> 31 : 0u;
  const uint32_t next = w < words - 1 ? bits[t + 1] & 1u : 0u;      // (bit 0 of the last word is inside the mask)
  *open = prev & x & 1u;
  *ends = x & ~((x >> 1) | (next << 31));
  return x & ~((x << 1) | prev);
}

__global__ void __launch_bounds__(kRsBlock) mask_runs_bounds_kernel(const int32_t *__restrict__ base,
                                                                   const int32_t *__restrict__ total, int n_inst,
                                                                   int64_t words, int64_t *__restrict__ bounds) {
  for (int64_t k = blockIdx.x * static_cast<int64_t>(kRsBlock) + threadIdx.x; k <= n_inst;
       k += static_cast<int64_t>(gridDim.x) * kRsBlock)
    bounds[k] = words == 0 ? 0 : (k < n_inst ? base[k * words] : *total);
}

// runs are counted where they start; the ends before word t are the starts before it less the run that is
// still open at its first bit
__global__ void __launch_bounds__(kRsBlock) mask_runs_fill_kernel(const uint32_t *__restrict__ bits, int64_t tw,
                                                                 int64_t words, int tail,
                                                                 const int32_t *__restrict__ base,
                                                                 int32_t *__restrict__ starts,
                                                                 int32_t *__restrict__ ends, int64_t capacity) {
  for (int64_t t = blockIdx.x * static_cast<int64_t>(kRsBlock) + threadIdx.x; t < tw;
       t += static_cast<int64_t>(gridDim.x) * kRsBlock) {
    const int64_t w = t % words;
    uint32_t open, e;
    uint32_t s = runs_word(bits, t, w, words, tail, &open, &e);
    int64_t at = base[t];
    for (; s; s &= s - 1, ++at)
      if (at >= 0 && at < capacity) starts[at] = static_cast<int32_t>(32 * w + (__ffs(s) - 1));
    at = static_cast<int64_t>(base[t]) - open;
    for (; e; e &= e - 1, ++at)
      if (at >= 0 && at < capacity) ends[at] = static_cast<int32_t>(32 * w + __ffs(e));
  }
}

struct MaskRunsWs {
  int32_t *base, *total;
  void *scan_ws;
  size_t scan_bytes;
};

static bool mask_runs_in_range(int n_inst, int64_t n_points) {
  // (the run numbers are int32: at most ceil(n_points / 2) runs per row)
  return n_inst >= 0 && n_points >= 0 && n_points < (1LL << 31) &&
         static_cast<int64_t>(n_inst) * ((n_points + 1) / 2) < (1LL << 31);
}

static size_t mask_runs_bytes(int n_inst, int64_t n_points) {
  const int64_t tw = static_cast<int64_t>(n_inst) * ((n_points + 31) / 32);
  return align_up(static_cast<size_t>(tw > 0 ? tw : 1) * 4) + align_up(scan_workspace_bytes(tw)) + align_up(64 * 4) + 256;
}

static bool mask_runs_carve(void *ws, size_t ws_bytes, int n_inst, int64_t n_points, MaskRunsWs *m) {
  if (ws == nullptr || ws_bytes < mask_runs_bytes(n_inst, n_points)) return false;
  const int64_t tw = static_cast<int64_t>(n_inst) * ((n_points + 31) / 32);
  Workspace a(ws, ws_bytes);
  m->base = a.take<int32_t>(static_cast<size_t>(tw > 0 ? tw : 1));
  m->scan_bytes = scan_workspace_bytes(tw);
  m->scan_ws = a.take<char>(m->scan_bytes);
  m->total = a.take<int32_t>(64);
  return m->total != nullptr;
}

}  // namespace sg

using namespace sg;

extern "C" {

size_t sg_grid_downsample_workspace_bytes(int n) {
  if (n < 0) return 0;
  const size_t nn = static_cast<size_t>(n > 0 ? n : 1), cap = static_cast<size_t>(table_cap(n));
  return 2 * align_up(cap * 4) + align_up(cap * 8) + 2 * align_up(nn * 4) + align_up(scan_workspace_bytes(n)) + 256;
}

int sg_grid_downsample(const float *xyz, int n, double voxel, int pick, int32_t *sample_ids, int32_t *inverse,
                       int32_t *meta, void *ws, size_t ws_bytes, sg_stream_t stream_) {
  SG_REQUIRE(n >= 0 && voxel > 0.0 && voxel <= 1.7976931348623157e308 && meta != nullptr &&
                 (pick == SG_PICK_FIRST || pick == SG_PICK_CENTER),
             "sg_grid_downsample: bad arguments (n=%d voxel=%g pick=%d)", n, voxel, pick);
  SG_REQUIRE(n == 0 || (xyz != nullptr && sample_ids != nullptr && inverse != nullptr), "sg_grid_downsample: null array");
  if (ws == nullptr || ws_bytes < sg_grid_downsample_workspace_bytes(n)) {
    set_error("sg_grid_downsample: workspace too small");
    return SG_ERR_WORKSPACE;
  }
  hipStream_t stream = as_stream(stream_);
  const size_t nn = static_cast<size_t>(n > 0 ? n : 1);
  DsArgs a;
  a.xyz = xyz, a.n = n, a.cap = table_cap(n), a.voxel = voxel, a.pick = pick, a.flags = meta + 1;
  Workspace w(ws, ws_bytes);
  a.owner = w.take<int32_t>(a.cap);
  a.best_idx = w.take<uint32_t>(a.cap);
  a.best_d2 = w.take<unsigned long long>(a.cap);
  a.slot_of = w.take<uint32_t>(nn);
  a.pos = w.take<int32_t>(nn);
  const size_t sbytes = scan_workspace_bytes(n);
  void *sws = w.take<char>(sbytes);
  SG_REQUIRE(sws != nullptr, "sg_grid_downsample: workspace too small");
  FillList f;
  f.add(meta, 8, 0);
  if (n > 0) {
    f.add(a.owner, static_cast<size_t>(a.cap) * 4, 0xff);
    f.add(a.best_idx, static_cast<size_t>(a.cap) * 4, 0xff);
    f.add(a.best_d2, static_cast<size_t>(a.cap) * 8, 0xff);
  }
  fill_many(f, stream);
  if (n == 0) return check_launch("sg_grid_downsample");
  const int grid = grid_for(n, kRsBlock, 4096);
  rs_validate_kernel<<<grid, kRsBlock, 0, stream>>>(xyz, n, voxel, kRsCellLimit, 1, 1, meta + 1);
  ds_insert_kernel<<<grid, kRsBlock, 0, stream>>>(a);
  if (pick == SG_PICK_CENTER) ds_select_kernel<<<grid, kRsBlock, 0, stream>>>(a);
  int32_t *pos = a.pos;
  const int rc = exclusive_scan([a] __device__(int64_t i) { return ds_is_rep(a, i); },
                                [pos] __device__(int64_t i, int v) { pos[i] = v; }, n, meta, sws, sbytes, stream);
  if (rc != SG_OK) return rc;
  ds_emit_kernel<<<grid, kRsBlock, 0, stream>>>(a, sample_ids, inverse);
  return check_launch("sg_grid_downsample");
}

double sg_nearest_default_cell(const double *lo, const double *hi, int64_t n_src) {
  if (lo == nullptr || hi == nullptr || n_src < 1) return 1.0;
  double vol = 1.0, reach = 0.0;
  int dims = 0;
  for (int k = 0; k < 3; ++k) {
    const double e = hi[k] - lo[k];
    if (e > 0.0 && e <= 1.7976931348623157e308) vol *= e, ++dims;
    const double m = fabs(lo[k]) > fabs(hi[k]) ? fabs(lo[k]) : fabs(hi[k]);
    if (m > reach && m <= 1.7976931348623157e308) reach = m;
  }
  double cell = dims == 0 ? 1.0 : pow(2.0 * vol / static_cast<double>(n_src), 1.0 / dims);
  if (!(cell > 0.0) || !(cell <= 1.7976931348623157e308)) cell = 1.0;
  const double floor_cell = reach / 536870912.0;      // 2^29: the cells of the whole box stay inside the grid's range
  return cell > floor_cell ? cell : floor_cell;
}

size_t sg_nearest_grid_bytes(int n_src) { return n_src < 0 ? 0 : nn_grid_bytes(n_src); }

int sg_nearest_build(const float *src, int n_src, double cell, void *grid, size_t grid_bytes, int32_t *meta,
                     sg_stream_t stream_) {
  SG_REQUIRE(n_src >= 1 && src != nullptr && meta != nullptr && cell > 0.0 && cell <= 1.7976931348623157e308,
             "sg_nearest_build: bad arguments (n_src=%d cell=%g)", n_src, cell);
  NnGrid g;
  if (!nn_carve(grid, grid_bytes, n_src, &g)) {
    set_error("sg_nearest_build: grid buffer too small");
    return SG_ERR_WORKSPACE;
  }
  hipStream_t stream = as_stream(stream_);
  FillList f;
  f.add(meta, 8, 0);
  f.add(g.owner, static_cast<size_t>(g.cap) * 4, 0xff);
  f.add(g.count, static_cast<size_t>(g.cap) * 4, 0);
  fill_many(f, stream);
  const int rc = nn_grid_build(src, n_src, cell, g, meta + 1, 4096, stream);
  if (rc != SG_OK) return rc;
  return check_launch("sg_nearest_build");
}

size_t sg_nearest_query_workspace_bytes(int n_query) {
  return n_query < 0 ? 0 : align_up(static_cast<size_t>(n_query > 0 ? n_query : 1) * 4) + 256;
}

int sg_nearest_query(const float *src, int n_src, double cell, const void *grid, size_t grid_bytes, const float *query,
                     int n_query, double max_dist, int32_t *index, double *dist2, int32_t *meta, void *ws,
                     size_t ws_bytes, sg_stream_t stream_) {
  SG_REQUIRE(n_src >= 1 && src != nullptr && meta != nullptr && n_query >= 0 && cell > 0.0 &&
                 cell <= 1.7976931348623157e308 && max_dist == max_dist,
             "sg_nearest_query: bad arguments (n_src=%d n_query=%d cell=%g)", n_src, n_query, cell);
  SG_REQUIRE(n_query == 0 || (query != nullptr && index != nullptr), "sg_nearest_query: null array");
  NnGrid g;
  if (!nn_carve(const_cast<void *>(grid), grid_bytes, n_src, &g)) {
    set_error("sg_nearest_query: grid buffer too small");
    return SG_ERR_WORKSPACE;
  }
  if (ws == nullptr || ws_bytes < sg_nearest_query_workspace_bytes(n_query)) {
    set_error("sg_nearest_query: workspace too small");
    return SG_ERR_WORKSPACE;
  }
  hipStream_t stream = as_stream(stream_);
  FillList f;
  f.add(meta, 4, 0);                                           // [0] = queries on the work list; the flags stay
  fill_many(f, stream);
  if (n_query == 0) return check_launch("sg_nearest_query");
  int32_t *work = static_cast<int32_t *>(ws);
  nn_query_kernel<<<grid_for(n_query, kRsBlock, 4096), kRsBlock, 0, stream>>>(g, n_src, cell, query, n_query, max_dist,
                                                                            index, dist2, meta, work);
  nn_scan_kernel<<<grid_for(n_query, 1, 4096), kRsBlock, 0, stream>>>(src, n_src, query, n_query, max_dist, index,
                                                                     dist2, meta, work);
  return check_launch("sg_nearest_query");
}

int sg_mask_bits_gather(const uint32_t *bits, int n_inst, int64_t n_src, const int32_t *index, int64_t n_out,
                        uint32_t *out, int32_t *meta, sg_stream_t stream_) {
  SG_REQUIRE(n_inst >= 0 && n_src >= 0 && n_src < (1LL << 31) && n_out >= 0 && n_out < (1LL << 31),
             "sg_mask_bits_gather: bad arguments (n_inst=%d n_src=%lld n_out=%lld)", n_inst,
             static_cast<long long>(n_src), static_cast<long long>(n_out));
  hipStream_t stream = as_stream(stream_);
  if (meta != nullptr) {
    FillList f;
    f.add(meta, 4, 0);
    fill_many(f, stream);
  }
  if (n_inst == 0 || n_out == 0) return check_launch("sg_mask_bits_gather");
  SG_REQUIRE(index != nullptr && out != nullptr && (n_src == 0 || bits != nullptr), "sg_mask_bits_gather: null array");
  const int64_t chunks = (n_out + 63) / 64;
  mask_gather_kernel<<<grid_for(chunks, kRsBlock / kWave, 8192), kRsBlock, 0, stream>>>(
      bits, n_inst, n_src, (n_src + 31) / 32, index, n_out, (n_out + 31) / 32, out, meta);
  return check_launch("sg_mask_bits_gather");
}

size_t sg_mask_runs_workspace_bytes(int n_inst, int64_t n_points) {
  return mask_runs_in_range(n_inst, n_points) ? mask_runs_bytes(n_inst, n_points) : 0;
}

int sg_mask_runs_count(const uint32_t *bits, int n_inst, int64_t n_points, int64_t *bounds, void *ws, size_t ws_bytes,
                       sg_stream_t stream_) {
  if (!mask_runs_in_range(n_inst, n_points)) {
    set_error("sg_mask_runs_count: %d masks over %lld points outside the supported range (n_points < 2^31, "
              "n_inst * ceil(n_points / 2) < 2^31)", n_inst, static_cast<long long>(n_points));
    return SG_ERR_UNSUPPORTED;
  }
  SG_REQUIRE(bounds != nullptr, "sg_mask_runs_count: null array");
  MaskRunsWs m;
  if (!mask_runs_carve(ws, ws_bytes, n_inst, n_points, &m)) {
    set_error("sg_mask_runs_count: workspace too small");
    return SG_ERR_WORKSPACE;
  }
  hipStream_t stream = as_stream(stream_);
  const int64_t words = (n_points + 31) / 32, tw = n_inst * words;
  const int tail = static_cast<int>(n_points & 31);
  SG_REQUIRE(tw == 0 || bits != nullptr, "sg_mask_runs_count: null array");
  int32_t *base = m.base;
  const int rc = exclusive_scan(
      [bits, words, tail] __device__(int64_t t) {
        uint32_t open, e;
        return __popc(runs_word(bits, t, t % words, words, tail, &open, &e));
      },
      [base] __device__(int64_t t, int v) { base[t] = v; }, tw, m.total, m.scan_ws, m.scan_bytes, stream);
  if (rc != SG_OK) return rc;
  mask_runs_bounds_kernel<<<grid_for(n_inst + 1, kRsBlock, 1024), kRsBlock, 0, stream>>>(m.base, m.total, n_inst,
                                                                                      tw == 0 ? 0 : words, bounds);
  return check_launch("sg_mask_runs_count");
}

int sg_mask_runs_fill(const uint32_t *bits, int n_inst, int64_t n_points, const void *ws, size_t ws_bytes,
                      int32_t *starts, int32_t *ends, int64_t capacity, sg_stream_t stream_) {
  if (!mask_runs_in_range(n_inst, n_points)) {
    set_error("sg_mask_runs_fill: %d masks over %lld points outside the supported range", n_inst,
              static_cast<long long>(n_points));
    return SG_ERR_UNSUPPORTED;
  }
  SG_REQUIRE(capacity >= 0 && (capacity == 0 || (starts != nullptr && ends != nullptr)), "sg_mask_runs_fill: bad arguments");
  MaskRunsWs m;
  if (!mask_runs_carve(const_cast<void *>(ws), ws_bytes, n_inst, n_points, &m)) {
    set_error("sg_mask_runs_fill: workspace too small");
    return SG_ERR_WORKSPACE;
  }
  const int64_t words = (n_points + 31) / 32, tw = n_inst * words;
  if (tw == 0 || capacity == 0) return SG_OK;
  SG_REQUIRE(bits != nullptr, "sg_mask_runs_fill: null array");
  mask_runs_fill_kernel<<<grid_for(tw, kRsBlock, 8192), kRsBlock, 0, as_stream(stream_)>>>(
      bits, tw, words, static_cast<int>(n_points & 31), m.base, starts, ends, capacity);
  return check_launch("sg_mask_runs_fill");
}

}  // extern "C"
