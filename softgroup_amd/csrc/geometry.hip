// geometry.hip -- superpoints for clouds that ship none: the exact k nearest neighbours of every point (sg_knn),
// normal and curvature per point (sg_point_normals) and the connected components of "same smooth surface" links
// (sg_grow_segments).  The reference has no counterpart of any of them.  All three are opt-in; the rules are stated
// in include/softgroup_hip.h and softgroup_amd.ops.geometry's numpy twins are the definition.
//
// knn      the hashed grid of point_grid.h (the one sg_nearest_build makes), then one THREAD per query, the queries
//          taken in the grid's cell order: the 64 lanes of a wave sit in the same or in adjacent cells, so they probe
//          the same slots, read the same runs of `sorted` (one fetch serves the wave) and leave their loops
//          together.  A thread keeps its k best (d2, j) as a sorted list in LDS, laid out [slot][thread] so that the
//          lanes of a wave touch consecutive words: 128 threads x 32 entries x 12 bytes = 48 KB, below the 64 KB a
//          kernel gets without asking and three workgroups to a CU's 160 KB -- that is why SG_KNN_MAX_K is 32 and
//          not 64 (96 KB: one workgroup per CU, four waves to hide every probe's latency).  A wave per query with
//          a wave-wide selection was the alternative: it needs a merge of 64 new candidates into the list per step
//          (a bitonic network of three-word keys over ds_bpermute / DPP), and with about 10 k candidates per list
//          entry the insertions a thread really performs are few: after the first k they happen with probability
//          k / (candidates seen).  Registers cannot hold the list: it is indexed by a run-time position.
//          The walk visits the shells of cells at Chebyshev distance 0 .. SG_KNN_MAX_SHELL and stops after shell R
//          once the list is full and its k-th d2 < (R cell)^2 (1 - 2^-18) -- the rule of nn_query_kernel at the k-th
//          place.  An undecided query goes onto the work list; knn_scan_kernel answers it with one wave: every lane
//          keeps the k best of its share of ALL points (the same list code), then k rounds of a wave-wide minimum
//          over the lanes' list heads write the row in (d2, j) order.
// normals  one thread per point, two passes over its list (centroid, covariance) in double in list order, then
//          kJacobiSweeps cyclic Jacobi sweeps on the 3 x 3 matrix in registers (fully unrolled, no indexing).
// grow     the union-find of union_find.h over the listed pairs that pass the link test, flatten, sizes by integer
//          atomicAdd at the roots, survivors numbered by a scan over the roots in index order (= ascending smallest
//          point), one pass that labels and absorbs.
//
// Integer and IEEE double arithmetic (-ffp-contract=off), selection by comparisons and integer atomics only: two
// calls on the same input give the same bytes (of sg_point_normals too: it has no atomics on its outputs).
//
// Bounds that do not depend on the data: a probe loop ends after `cap` probes, a shell walk after SG_KNN_MAX_SHELL
// shells, a list insertion after SG_KNN_MAX_K steps, a find after N + 1 steps, a union after 2 N + 2 rounds, the
// eigen-solver after kJacobiSweeps sweeps.  Every index read from memory (neighbour ids, slot contents, cell starts
// and counts, work-list entries, roots) is range-checked before it addresses anything.  No kernel here caps its
// grid except knn_scan_kernel (kKnnScanBlocks workgroups stride over the work list).
#include "point_grid.h"
#include "union_find.h"

namespace sg {

constexpr int kGeoBlock = 256;
constexpr int kKnnBlock = 128;
constexpr int kKnnScanBlock = 64;                    // one wave: its lanes share nothing but the final selection
constexpr int kKnnScanBlocks = 2048;
constexpr int kKnnMaxK = SG_KNN_MAX_K;
constexpr int kKnnMaxShell = SG_KNN_MAX_SHELL;
constexpr int kJacobiSweeps = 8;
constexpr int kGeoMaxListed = 4096;                  // entries per neighbour list (normals, growth)
constexpr int kNoBlockCap = 0x7FFFFFFF;
static_assert(kKnnBlock * kKnnMaxK * 12 <= 65536, "the lists of a workgroup fit the LDS a kernel gets by default");

__device__ __forceinline__ double geo_inf() { return __longlong_as_double(0x7FF0000000000000LL); }

// ---- knn ---------------------------------------------------------------------------------------------------------
// The k best (d2, j) of one thread, ascending, in LDS at [slot * B + tid].
template <int B>
struct KnnList {
  double *d;
  int32_t *j;
  int k, count;
  double wd;                       // the k-th entry once the list is full
  int32_t wj;
  __device__ __forceinline__ void init(double *lds, int k_, int tid) {
    d = lds + tid, j = reinterpret_cast<int32_t *>(lds + static_cast<size_t>(k_) * B) + tid;
    k = k_, count = 0, wd = geo_inf(), wj = INT32_MAX;
  }
  __device__ __forceinline__ void push(double d2, int32_t id) {
    if (count == k && !(d2 < wd || (d2 == wd && id < wj))) return;
    int p = count < k ? count : k - 1;
    for (int it = 0; it < kKnnMaxK && p > 0; ++it) {
      const double pd = d[(p - 1) * B];
      const int32_t pj = j[(p - 1) * B];
      if (pd < d2 || (pd == d2 && pj < id)) break;
      d[p * B] = pd, j[p * B] = pj;
      --p;
    }
    d[p * B] = d2, j[p * B] = id;
    if (count < k) ++count;
    if (count == k) wd = d[(k - 1) * B], wj = j[(k - 1) * B];
  }
};

struct KnnArgs {
  const float *xyz;
  int64_t n;
  int k, r_md;                     // r_md >= 0: max_dist reaches no farther than r_md shells, which the walk visits
  double cell, max_dist, md2;
  int32_t *idx;                    // [n, k]
  double *d2;                      // [n, k]
  int32_t *meta;                   // [0] queries on the work list, [1] flags
  int32_t *work;                   // [n]
  NnGrid g;
};

// One thread per position of `sorted` (= per query, in cell order).
__global__ void __launch_bounds__(kKnnBlock) knn_walk_kernel(KnnArgs a) {
  extern __shared__ double knn_lds[];
  if (a.meta[1] != 0) return;                                     // invalid input: nothing is written
  const int64_t t = blockIdx.x * static_cast<int64_t>(kKnnBlock) + threadIdx.x;
  if (t >= a.n) return;
  const float4 me = a.g.sorted[t];
  const int32_t q = __float_as_int(me.w);
  if (q < 0 || q >= a.n) return;                                  // (the build wrote a permutation: never)
  KnnList<kKnnBlock> best;
  best.init(knn_lds, a.k, threadIdx.x);
  const float p[3] = {me.x, me.y, me.z};
  const double qx = p[0], qy = p[1], qz = p[2];
  const bool limited = a.max_dist >= 0.0;
  int32_t c[3];
  bool done = false;
  if (cell_of(p, a.cell, kNnCellLimit, c)) {
    const int last = a.r_md >= 0 ? a.r_md : kKnnMaxShell;         // (<= kKnnMaxShell: the host checked)
    for (int R = 0; R <= last && R <= kKnnMaxShell && !done; ++R) {
      for (int dz = -R; dz <= R; ++dz)
        for (int dy = -R; dy <= R; ++dy) {
          // inside the shell's box only the two end cells of a row belong to the shell
          const int step = (abs(dz) == R || abs(dy) == R || R == 0) ? 1 : 2 * R;
          for (int dx = -R; dx <= R; dx += step) {
            const int32_t cx = c[0] + dx, cy = c[1] + dy, cz = c[2] + dz;      // |c| < 2^30: no overflow
            uint64_t s = cell_hash(cx, cy, cz) & static_cast<uint64_t>(a.g.cap - 1);
            for (int64_t probe = 0; probe < a.g.cap; ++probe) {
              const int32_t cnt = a.g.count[s];
              if (cnt <= 0) break;                                           // a free slot ends the chain
              const int4 key = a.g.key[s];
              if (key.x == cx && key.y == cy && key.z == cz) {
                if (key.w >= 0 && static_cast<int64_t>(key.w) + cnt <= a.n) {
                  for (int32_t u = key.w; u < key.w + cnt; ++u) {
                    const float4 v = a.g.sorted[u];
                    const int32_t j = __float_as_int(v.w);
                    if (j < 0 || j >= a.n || j == q) continue;
                    const double d2 = nn_d2(qx, qy, qz, v.x, v.y, v.z);
                    if (limited && d2 > a.md2) continue;
                    best.push(d2, j);
                  }
                }
                break;
              }
              s = (s + 1) & static_cast<uint64_t>(a.g.cap - 1);
            }
          }
        }
      const double bound = (static_cast<double>(R) * a.cell) * (static_cast<double>(R) * a.cell) * kNnStopMargin;
      done = best.count == a.k && (R == 0 ? best.wd == 0.0 : best.wd < bound);
    }
    if (a.r_md >= 0) done = true;                                 // every cell within max_dist has been visited
  }
  if (done) {
    int32_t *oi = a.idx + static_cast<int64_t>(q) * a.k;
    double *od = a.d2 + static_cast<int64_t>(q) * a.k;
    for (int s = 0; s < a.k && s < kKnnMaxK; ++s) {
      const bool have = s < best.count;
      oi[s] = have ? best.j[s * kKnnBlock] : -1;
      od[s] = have ? best.d[s * kKnnBlock] : geo_inf();
    }
  } else {
    const int32_t w = atomicAdd(&a.meta[0], 1);
    if (w >= 0 && w < a.n) a.work[w] = q;
  }
}

// One wave per listed query: every point, the same (d2, j) order.
__global__ void __launch_bounds__(kKnnScanBlock) knn_scan_kernel(KnnArgs a) {
  extern __shared__ double knn_lds[];
  if (a.meta[1] != 0) return;
  const int lane = threadIdx.x;
  int64_t n_work = a.meta[0];
  n_work = n_work < 0 ? 0 : (n_work > a.n ? a.n : n_work);
  const bool limited = a.max_dist >= 0.0;
  for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {      // (wave-uniform)
    const int64_t q = a.work[w];
    if (q < 0 || q >= a.n) continue;
    const double qx = a.xyz[3 * q], qy = a.xyz[3 * q + 1], qz = a.xyz[3 * q + 2];
    KnnList<kKnnScanBlock> best;
    best.init(knn_lds, a.k, lane);
    for (int64_t j = lane; j < a.n; j += kKnnScanBlock) {
      if (j == q) continue;
      const double d2 = nn_d2(qx, qy, qz, a.xyz[3 * j], a.xyz[3 * j + 1], a.xyz[3 * j + 2]);
      if (limited && d2 > a.md2) continue;
      best.push(d2, static_cast<int32_t>(j));
    }
    int head = 0;
    int32_t *oi = a.idx + q * a.k;
    double *od = a.d2 + q * a.k;
    for (int s = 0; s < a.k && s < kKnnMaxK; ++s) {               // (wave-uniform: all lanes take every round)
      const bool have = head < best.count;
      const double md = have ? best.d[head * kKnnScanBlock] : geo_inf();
      const int32_t mj = have ? best.j[head * kKnnScanBlock] : INT32_MAX;
      double bd = md;
      int32_t bj = mj;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double od2 = __shfl_xor(bd, o, 64);
        const int32_t oj = __shfl_xor(bj, o, 64);
        if (od2 < bd || (od2 == bd && oj < bj)) bd = od2, bj = oj;
      }
      if (have && mj == bj) ++head;                               // (an index sits in one lane's list only)
      if (lane == 0) {
        const bool any = bj != INT32_MAX;
        oi[s] = any ? bj : -1;
        od[s] = any ? bd : geo_inf();
      }
    }
  }
}

static size_t knn_layout(int64_t n, void *base, size_t bytes, NnGrid *g, int32_t **work) {
  const size_t gb = align_up(nn_grid_bytes(n)), wb = align_up(static_cast<size_t>(n > 0 ? n : 1) * 4);
  if (base != nullptr) {
    if (bytes < gb + wb || !nn_carve(base, gb, n, g)) return 0;
    Workspace rest(static_cast<char *>(base) + gb, bytes - gb);
    *work = rest.take<int32_t>(static_cast<size_t>(n > 0 ? n : 1));
    if (*work == nullptr) return 0;
  }
  return gb + wb + 256;
}

// ---- normals -----------------------------------------------------------------------------------------------------
// One Jacobi rotation that zeroes a_pq of a symmetric 3 x 3 matrix (r = the third index); v = the eigenvector
// columns.  t is the smaller root of t^2 + 2 theta t - 1 = 0; a theta that overflows gives t = 0.
#define SG_JACOBI_ROT(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q)                         \
  if (apq != 0.0) {                                                                                  \
    const double theta = (aqq - app) / (2.0 * apq);                                                  \
    const double tt = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));              \
    const double cc = 1.0 / sqrt(tt * tt + 1.0), ss = tt * cc;                                       \
    app -= tt * apq, aqq += tt * apq, apq = 0.0;                                                     \
    double u_ = arp, w_ = arq;                                                                       \
    arp = cc * u_ - ss * w_, arq = ss * u_ + cc * w_;                                                \
    u_ = v0p, w_ = v0q, v0p = cc * u_ - ss * w_, v0q = ss * u_ + cc * w_;                            \
    u_ = v1p, w_ = v1q, v1p = cc * u_ - ss * w_, v1q = ss * u_ + cc * w_;                            \
    u_ = v2p, w_ = v2q, v2p = cc * u_ - ss * w_, v2q = ss * u_ + cc * w_;                            \
  }

__global__ void __launch_bounds__(kGeoBlock) normals_kernel(const float *__restrict__ xyz, int64_t n,
                                                           const int32_t *__restrict__ nbr, int k, int min_nb,
                                                           float *__restrict__ normals, float *__restrict__ curvature,
                                                           int32_t *__restrict__ meta) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kGeoBlock) + threadIdx.x;
  if (i >= n) return;
  const int32_t *row = nbr + i * k;
  bool bad = false;
  // the support: i itself, then its valid neighbours in list order
  double sx = xyz[3 * i], sy = xyz[3 * i + 1], sz = xyz[3 * i + 2];
  int valid = 0;
  for (int m = 0; m < k; ++m) {
    const int32_t j = row[m];
    if (j < -1 || j >= n) bad = true;
    if (j < 0 || j >= n) continue;
    sx += static_cast<double>(xyz[3 * static_cast<int64_t>(j)]);
    sy += static_cast<double>(xyz[3 * static_cast<int64_t>(j) + 1]);
    sz += static_cast<double>(xyz[3 * static_cast<int64_t>(j) + 2]);
    ++valid;
  }
  if (bad) atomicOr(&meta[1], SG_GEOMETRY_FLAG_INDEX);
  float out[4] = {0.f, 0.f, 0.f, 0.f};
  if (valid >= min_nb) {
    const double cnt = static_cast<double>(valid + 1);
    const double mx = sx / cnt, my = sy / cnt, mz = sz / cnt;
    double dx = static_cast<double>(xyz[3 * i]) - mx, dy = static_cast<double>(xyz[3 * i + 1]) - my,
           dz = static_cast<double>(xyz[3 * i + 2]) - mz;
    double cxx = dx * dx, cxy = dx * dy, cxz = dx * dz, cyy = dy * dy, cyz = dy * dz, czz = dz * dz;
    for (int m = 0; m < k; ++m) {
      const int32_t j = row[m];
      if (j < 0 || j >= n) continue;
      dx = static_cast<double>(xyz[3 * static_cast<int64_t>(j)]) - mx;
      dy = static_cast<double>(xyz[3 * static_cast<int64_t>(j) + 1]) - my;
      dz = static_cast<double>(xyz[3 * static_cast<int64_t>(j) + 2]) - mz;
      cxx += dx * dx, cxy += dx * dy, cxz += dx * dz, cyy += dy * dy, cyz += dy * dz, czz += dz * dz;
    }
    const double tr = (cxx + cyy) + czz;
    if (tr > 0.0 && tr < geo_inf()) {
      // eigenvalues of C / tr: the ratio that is the curvature and the vectors do not change
      double a00 = cxx / tr, a01 = cxy / tr, a02 = cxz / tr, a11 = cyy / tr, a12 = cyz / tr, a22 = czz / tr;
      double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
      for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        SG_JACOBI_ROT(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21)
        SG_JACOBI_ROT(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22)
        SG_JACOBI_ROT(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22)
      }
      double l0, nx, ny, nz;
      if (a00 <= a11 && a00 <= a22)
        l0 = a00, nx = v00, ny = v10, nz = v20;
      else if (a11 <= a22)
        l0 = a11, nx = v01, ny = v11, nz = v21;
      else
        l0 = a22, nx = v02, ny = v12, nz = v22;
      const double len = sqrt((nx * nx + ny * ny) + nz * nz);
      const double sum = (a00 + a11) + a22;
      if (len > 0.0) {
        nx /= len, ny /= len, nz /= len;
        // the component of greatest magnitude is positive, the lowest axis among equal magnitudes
        double lead = nx;
        if (fabs(ny) > fabs(lead)) lead = ny;
        if (fabs(nz) > fabs(lead)) lead = nz;
        if (lead < 0.0) nx = -nx, ny = -ny, nz = -nz;
        out[0] = static_cast<float>(nx), out[1] = static_cast<float>(ny), out[2] = static_cast<float>(nz);
        l0 = l0 > 0.0 ? l0 : 0.0;
        out[3] = sum > 0.0 ? static_cast<float>(l0 / sum) : 0.f;
      }
    }
  }
  normals[3 * i] = out[0], normals[3 * i + 1] = out[1], normals[3 * i + 2] = out[2];
  curvature[i] = out[3];
  const bool none = out[0] == 0.f && out[1] == 0.f && out[2] == 0.f;
  const uint64_t m = __ballot(none);
  if (none && mask_prefix(m) == 0) atomicAdd(&meta[0], __popcll(m));
}

// ---- growth ------------------------------------------------------------------------------------------------------
struct GrowArgs {
  const int32_t *nbr;
  const double *nbr_d2;            // null: no distance test
  const float *normals, *curvature;      // curvature null: no curvature test
  int64_t n;
  int k, min_size, absorb;
  double cos_thr, md2;
  float max_curv;
  int32_t *sp, *meta;              // meta: [0] segments, [1] flags, [2] components
  int32_t *parent, *root, *size, *outidx;
};

__device__ __forceinline__ bool grow_has_normal(const float *__restrict__ nm, int64_t i) {
  return nm[3 * i] != 0.f || nm[3 * i + 1] != 0.f || nm[3 * i + 2] != 0.f;
}

__global__ void __launch_bounds__(kGeoBlock) grow_init_kernel(GrowArgs a) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kGeoBlock) + threadIdx.x;
  if (i >= a.n) return;
  a.parent[i] = static_cast<int32_t>(i);
  a.size[i] = 0;
}

// One thread per point: the entries of its own list that pass the link test (the union makes the edge symmetric).
__global__ void __launch_bounds__(kGeoBlock) grow_edges_kernel(GrowArgs a) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kGeoBlock) + threadIdx.x;
  if (i >= a.n) return;
  int flags = 0;
  const bool mine = grow_has_normal(a.normals, i) && (a.curvature == nullptr || a.curvature[i] <= a.max_curv);
  const double nx = a.normals[3 * i], ny = a.normals[3 * i + 1], nz = a.normals[3 * i + 2];
  for (int m = 0; m < a.k; ++m) {
    const int32_t j = a.nbr[i * a.k + m];
    if (j < -1 || j >= a.n) flags |= SG_GEOMETRY_FLAG_INDEX;
    if (j < 0 || j >= a.n || j == i || !mine) continue;
    if (!grow_has_normal(a.normals, j)) continue;
    if (a.curvature != nullptr && !(a.curvature[j] <= a.max_curv)) continue;
    if (a.nbr_d2 != nullptr && !(a.nbr_d2[i * a.k + m] <= a.md2)) continue;
    const double dot = (nx * static_cast<double>(a.normals[3 * static_cast<int64_t>(j)]) +
                        ny * static_cast<double>(a.normals[3 * static_cast<int64_t>(j) + 1])) +
                       nz * static_cast<double>(a.normals[3 * static_cast<int64_t>(j) + 2]);
    if (!(fabs(dot) >= a.cos_thr)) continue;
    if (!uf_unite(a.parent, static_cast<int32_t>(i), j, a.n)) flags |= SG_GEOMETRY_FLAG_INTERNAL;
  }
  if (flags) atomicOr(&a.meta[1], flags);
}

// every point's root (into an array of its own: path halving may still rewrite `parent`), sizes at the roots
__global__ void __launch_bounds__(kGeoBlock) grow_flatten_kernel(GrowArgs a) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kGeoBlock) + threadIdx.x;
  if (i >= a.n) return;
  const int32_t r = uf_find(a.parent, static_cast<int32_t>(i), a.n);
  a.root[i] = r;
  if (r < 0 || r >= a.n) {
    atomicOr(&a.meta[1], SG_GEOMETRY_FLAG_INTERNAL);
    return;
  }
  atomicAdd(&a.size[r], 1);
  if (r == i) atomicAdd(&a.meta[2], 1);
}

struct GrowKeepIn {
  const int32_t *root, *size;
  int min_size;
  __device__ int operator()(int64_t i) const { return (root[i] == i && size[i] >= min_size) ? 1 : 0; }
};
struct GrowKeepOut {
  GrowKeepIn in;
  int32_t *outidx;
  __device__ void operator()(int64_t i, int v) const { outidx[i] = in(i) ? v : -1; }
};

// the number of point j's component, -1 when it has none (or j is no point)
__device__ __forceinline__ int32_t grow_label(const GrowArgs &a, int64_t j, int32_t n_seg) {
  if (j < 0 || j >= a.n) return -1;
  const int32_t r = a.root[j];
  if (r < 0 || r >= a.n) return -1;
  const int32_t o = a.outidx[r];
  return (o >= 0 && o < n_seg) ? o : -1;
}

// labels, and for a point of a small component the first entry of its own list that lies in a numbered one; it reads
// root / outidx only, the labels from before the pass
__global__ void __launch_bounds__(kGeoBlock) grow_label_kernel(GrowArgs a) {
  const int64_t i = blockIdx.x * static_cast<int64_t>(kGeoBlock) + threadIdx.x;
  if (i >= a.n) return;
  int32_t n_seg = a.meta[0];
  n_seg = n_seg < 0 ? 0 : n_seg;
  int32_t l = grow_label(a, i, n_seg);
  if (l < 0 && a.absorb)
    for (int m = 0; m < a.k && l < 0; ++m) l = grow_label(a, a.nbr[i * a.k + m], n_seg);
  a.sp[i] = l;
}

static size_t grow_layout(int64_t n, void *base, size_t bytes, GrowArgs *a, void **scan_ws, size_t *scan_bytes) {
  const size_t nn = static_cast<size_t>(n > 0 ? n : 1), sb = scan_workspace_bytes(static_cast<int64_t>(nn));
  const size_t need = 4 * align_up(nn * 4) + align_up(sb) + 256;
  if (base != nullptr) {
    if (bytes < need) return 0;
    Workspace w(base, bytes);
    a->parent = w.take<int32_t>(nn), a->root = w.take<int32_t>(nn);
    a->size = w.take<int32_t>(nn), a->outidx = w.take<int32_t>(nn);
    *scan_ws = w.take<char>(sb), *scan_bytes = sb;
    if (*scan_ws == nullptr) return 0;
  }
  return need;
}

inline unsigned geo_blocks(int64_t items, int per_block) {
  return static_cast<unsigned>(items <= 0 ? 1 : (items + per_block - 1) / per_block);
}

}  // namespace sg

using namespace sg;

extern "C" {

double sg_knn_default_cell(const double *lo, const double *hi, int64_t n, int k) {
  if (lo == nullptr || hi == nullptr || n < 1) return 1.0;
  if (k < 2) k = 2;
  double vol = 1.0, reach = 0.0;
  int dims = 0;
  for (int d = 0; d < 3; ++d) {
    const double e = hi[d] - lo[d];
    if (e > 0.0 && e <= 1.7976931348623157e308) vol *= e, ++dims;
    const double m = fabs(lo[d]) > fabs(hi[d]) ? fabs(lo[d]) : fabs(hi[d]);
    if (m > reach && m <= 1.7976931348623157e308) reach = m;
  }
  double cell = dims == 0 ? 1.0 : pow(0.5 * static_cast<double>(k) * vol / static_cast<double>(n), 1.0 / dims);
  if (!(cell > 0.0) || !(cell <= 1.7976931348623157e308)) cell = 1.0;
  const double floor_cell = reach / 536870912.0;      // 2^29: the cells of the whole box stay inside the grid's range
  return cell > floor_cell ? cell : floor_cell;
}

static bool knn_in_range(int64_t n, int k) { return n >= 0 && n < (1LL << 31) && k >= 1 && k <= kKnnMaxK; }

size_t sg_knn_workspace_bytes(int64_t n, int k) {
  if (!knn_in_range(n, k)) return 0;
  return knn_layout(n, nullptr, 0, nullptr, nullptr);
}

int sg_knn(const float *xyz, int64_t n, int k, double cell, double max_dist, int32_t *idx, double *d2, int32_t *meta,
           void *ws, size_t ws_bytes, sg_stream_t stream_) {
  if (!knn_in_range(n, k)) {
    set_error("sg_knn: n %lld, k %d outside the supported range (0 <= n < 2^31, 1 <= k <= %d)",
              static_cast<long long>(n), k, kKnnMaxK);
    return SG_ERR_UNSUPPORTED;
  }
  SG_REQUIRE(meta != nullptr && cell > 0.0 && cell <= 1.7976931348623157e308 && max_dist == max_dist,
             "sg_knn: bad arguments (cell %g, max_dist %g)", cell, max_dist);
  hipStream_t stream = as_stream(stream_);
  hipMemsetAsync(meta, 0, 4 * sizeof(int32_t), stream);
  if (n == 0) return check_launch("sg_knn");
  SG_REQUIRE(xyz != nullptr && idx != nullptr && d2 != nullptr, "sg_knn: null array");
  KnnArgs a;
  if (ws == nullptr || ws_bytes < sg_knn_workspace_bytes(n, k) || knn_layout(n, ws, ws_bytes, &a.g, &a.work) == 0) {
    set_error("sg_knn: workspace too small (%zu bytes, %zu needed)", ws_bytes, sg_knn_workspace_bytes(n, k));
    return SG_ERR_WORKSPACE;
  }
  a.xyz = xyz, a.n = n, a.k = k, a.cell = cell, a.idx = idx, a.d2 = d2, a.meta = meta;
  a.max_dist = max_dist >= 0.0 ? max_dist : -1.0;
  a.md2 = max_dist >= 0.0 ? max_dist * max_dist : -1.0;
  a.r_md = -1;
  if (max_dist >= 0.0) {
    // two points within max_dist differ by at most ceil(max_dist / cell) cells per axis; the factor covers the
    // roundings of the quotients
    const double shells = ceil(max_dist / cell * (1.0 + 1.0 / 1048576.0));
    if (shells <= static_cast<double>(kKnnMaxShell)) a.r_md = static_cast<int>(shells);
  }
  hipMemsetAsync(a.g.owner, 0xff, static_cast<size_t>(a.g.cap) * 4, stream);
  hipMemsetAsync(a.g.count, 0, static_cast<size_t>(a.g.cap) * 4, stream);
  const int rc = nn_grid_build(xyz, n, cell, a.g, meta + 1, kNoBlockCap, stream);
  if (rc != SG_OK) return rc;
  knn_walk_kernel<<<geo_blocks(n, kKnnBlock), kKnnBlock, static_cast<size_t>(k) * kKnnBlock * 12, stream>>>(a);
  const int64_t scan_blocks = n < kKnnScanBlocks ? n : kKnnScanBlocks;
  knn_scan_kernel<<<static_cast<unsigned>(scan_blocks), kKnnScanBlock, static_cast<size_t>(k) * kKnnScanBlock * 12,
                    stream>>>(a);
  return check_launch("sg_knn");
}

static bool geo_list_in_range(int64_t n, int k) { return n >= 0 && n < (1LL << 31) && k >= 1 && k <= kGeoMaxListed; }

int sg_point_normals(const float *xyz, int64_t n, const int32_t *nbr, int k, int min_neighbours, float *normals,
                     float *curvature, int32_t *meta, sg_stream_t stream_) {
  if (!geo_list_in_range(n, k)) {
    set_error("sg_point_normals: n %lld, k %d outside the supported range (0 <= n < 2^31, 1 <= k <= %d)",
              static_cast<long long>(n), k, kGeoMaxListed);
    return SG_ERR_UNSUPPORTED;
  }
  SG_REQUIRE(meta != nullptr && min_neighbours >= 0, "sg_point_normals: bad arguments (min_neighbours %d)",
             min_neighbours);
  hipStream_t stream = as_stream(stream_);
  hipMemsetAsync(meta, 0, 4 * sizeof(int32_t), stream);
  if (n == 0) return check_launch("sg_point_normals");
  SG_REQUIRE(xyz != nullptr && nbr != nullptr && normals != nullptr && curvature != nullptr,
             "sg_point_normals: null array");
  normals_kernel<<<geo_blocks(n, kGeoBlock), kGeoBlock, 0, stream>>>(xyz, n, nbr, k, min_neighbours, normals, curvature,
                                                                    meta);
  return check_launch("sg_point_normals");
}

size_t sg_grow_segments_workspace_bytes(int64_t n) {
  if (n < 0 || n >= (1LL << 31)) return 0;
  return grow_layout(n, nullptr, 0, nullptr, nullptr, nullptr);
}

int sg_grow_segments(const int32_t *nbr, const double *nbr_d2, int64_t n, int k, const float *normals,
                     const float *curvature, double cos_thr, float max_curvature, double max_dist, int min_size,
                     int absorb, int32_t *sp, int32_t *meta, void *ws, size_t ws_bytes, sg_stream_t stream_) {
  if (!geo_list_in_range(n, k)) {
    set_error("sg_grow_segments: n %lld, k %d outside the supported range (0 <= n < 2^31, 1 <= k <= %d)",
              static_cast<long long>(n), k, kGeoMaxListed);
    return SG_ERR_UNSUPPORTED;
  }
  SG_REQUIRE(meta != nullptr && cos_thr == cos_thr && max_dist == max_dist && min_size >= 1 &&
                 (absorb == 0 || absorb == 1) && (max_dist < 0.0 || nbr_d2 != nullptr) &&
                 (curvature == nullptr || max_curvature == max_curvature),
             "sg_grow_segments: bad arguments (cos_thr %g, max_dist %g, min_size %d, absorb %d)", cos_thr, max_dist,
             min_size, absorb);
  hipStream_t stream = as_stream(stream_);
  hipMemsetAsync(meta, 0, 4 * sizeof(int32_t), stream);
  if (n == 0) return check_launch("sg_grow_segments");
  SG_REQUIRE(nbr != nullptr && normals != nullptr && sp != nullptr, "sg_grow_segments: null array");
  GrowArgs a;
  void *scan_ws;
  size_t scan_bytes;
  if (ws == nullptr || grow_layout(n, ws, ws_bytes, &a, &scan_ws, &scan_bytes) == 0) {
    set_error("sg_grow_segments: workspace too small (%zu bytes, %zu needed)", ws_bytes,
              sg_grow_segments_workspace_bytes(n));
    return SG_ERR_WORKSPACE;
  }
  a.nbr = nbr, a.nbr_d2 = max_dist >= 0.0 ? nbr_d2 : nullptr, a.normals = normals, a.curvature = curvature;
  a.n = n, a.k = k, a.min_size = min_size, a.absorb = absorb;
  a.cos_thr = cos_thr, a.md2 = max_dist >= 0.0 ? max_dist * max_dist : -1.0, a.max_curv = max_curvature;
  a.sp = sp, a.meta = meta;
  const unsigned grid = geo_blocks(n, kGeoBlock);
  grow_init_kernel<<<grid, kGeoBlock, 0, stream>>>(a);
  grow_edges_kernel<<<grid, kGeoBlock, 0, stream>>>(a);
  grow_flatten_kernel<<<grid, kGeoBlock, 0, stream>>>(a);
  const GrowKeepIn keep{a.root, a.size, min_size};
  const int rc = exclusive_scan(keep, GrowKeepOut{keep, a.outidx}, n, meta, scan_ws, scan_bytes, stream);
  if (rc != SG_OK) return rc;
  grow_label_kernel<<<grid, kGeoBlock, 0, stream>>>(a);
  return check_launch("sg_grow_segments");
}

}  // extern "C"
