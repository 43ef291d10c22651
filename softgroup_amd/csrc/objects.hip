// objects.hip -- the object table of a mask list: population, axis-aligned box, centroid, centred second moments and
// colour means (sg_instance_moments), the extents of every mask along a table of directions and the direction of the
// smallest enclosing rectangle (sg_instance_extents), the semantic vote (sg_instance_class_hist).  The rules are
// stated in include/softgroup_hip.h; the reference has no counterpart.
//
// A workgroup owns one mask and one aligned chunk of kObjChunkWords words of its row and leaves at once when the
// chunk's words are all zero (a mask covers about 1 % of a cloud).  Grids are capped at kObjMaxBlocks and walked by
// block-uniform stride loops.
//
// Sums: the ORDER is the definition.  One lane adds the set bits of one word in ascending order; the 64 lanes of a
// wave combine by the xor butterfly (1, 2, 4, ...), which is the adjacent-pair tree (IEEE addition commutes); the two
// waves of a workgroup combine through LDS; a chunk stores one partial per quantity in a slab [n, chunks, kObjSlab]
// and a second kernel runs the same adjacent-pair tree over the chunks -- 64 chunks by the butterfly, the groups of
// 64 by a binary-counter stack, which is the tree padded with +0.0 to the next power of two.  A partial is never
// -0.0, so a skipped chunk counts as +0.0 exactly.  The centroid stays on the device between the two passes.
// No float atomics (-ffp-contract=off: every product and sum is rounded once).
//
// Extremes are order-free: 64-bit integer atomicMin / atomicMax on order-preserving keys of the doubles (the keys of
// det_eval.hip), one per workgroup per (angle, extreme).  The histogram uses integer atomics only.
//
// Every loop is bounded by an argument, every index is checked against n_points, the word count, the angle count or
// the class count before it addresses anything.  No workgroup waits for another one.
#include "common.h"

namespace sg {

constexpr int kObjChunkWords = 128;                   // 2^7 words = 4096 points per (mask, chunk) workgroup
constexpr int kObjMaxBlocks = 4096;                   // grid cap of the (mask, chunk) kernels, walked by a stride loop
constexpr int kObjSumBlock = kObjChunkWords;          // sums: one lane per word
constexpr int kObjExtBlock = 256;
constexpr int kObjMaxInst = 16384;
constexpr int kObjMaxAngles = 180;
constexpr int kObjMaxClasses = 256;
constexpr int kObjSlab = 16;                          // doubles per (mask, chunk): count, 6 sums, 3 minima, 3 maxima
constexpr int kObjLevels = 16;                        // stack of the tree over groups of 64 chunks (< 2^13 groups)
constexpr uint64_t kObjKeyMin0 = ~0ULL;               // identity of a min over keys
constexpr uint64_t kObjKeyMax0 = 0ULL;                // identity of a max over keys

// float64 -> uint64 key with the same order (negative: all bits flipped; non-negative: sign bit set)
__device__ __forceinline__ uint64_t obj_key(double d) {
  const uint64_t u = static_cast<uint64_t>(__double_as_longlong(d));
  return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}
__device__ __forceinline__ double obj_key_decode(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k ^ 0x8000000000000000ULL) : ~k;
  return __longlong_as_double(static_cast<long long>(u));
}
__device__ __forceinline__ double obj_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// the adjacent-pair tree over the 64 lanes of a wave; every lane ends with the root (EXEC full)
__device__ __forceinline__ double wave_tree_sum(double v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}

// the word of (mask m, word w), bits at and beyond n_points cleared; 0 outside the row
__device__ __forceinline__ uint32_t obj_word(const uint32_t *bits, int m, int64_t w, int64_t words, int64_t n_points) {
  if (w >= words) return 0u;
  uint32_t x = bits[static_cast<int64_t>(m) * words + w];
  const int tail = static_cast<int>(n_points & 31);
  if (w == words - 1 && tail) x &= (1u << tail) - 1u;
  return x;
}

// ---- sums ---------------------------------------------------------------------------------------------------------
struct MoArgs {
  const uint32_t *bits;                 // [n, words]
  const float *coords, *colors;         // [n_points, 3]; colors may be null
  const double *centroid;               // [n, 3] (pass 2)
  double *slab;                         // [n, chunks, kObjSlab]
  int32_t *flags;
  int64_t n_points, words, chunks;
  int n;
};

// PASS 1: slab = count, sum x y z, sum r g b, min x y z, max x y z.  PASS 2: slab[1 .. 6] = the six centred sums.
template <int PASS>
__global__ void __launch_bounds__(kObjSumBlock) moments_chunk_kernel(MoArgs a) {
  constexpr int kWaves = kObjSumBlock / 64;
  __shared__ double part[kWaves][12];
  __shared__ int part_cnt[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t items = static_cast<int64_t>(a.n) * a.chunks;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {          // (block-uniform)
    const int m = static_cast<int>(item / a.chunks);
    const int64_t w = (item - static_cast<int64_t>(m) * a.chunks) * kObjChunkWords + tid;
    const uint32_t word = obj_word(a.bits, m, w, a.words, a.n_points);
    double *out = a.slab + item * kObjSlab;
    if (!__syncthreads_or(word != 0u)) {                                      // (also the barrier before part is reused)
      if (PASS == 1 && tid == 0) out[0] = 0.0;
      continue;
    }
    double q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    double c[3] = {0.0, 0.0, 0.0};
    if (PASS == 2) c[0] = a.centroid[3 * m], c[1] = a.centroid[3 * m + 1], c[2] = a.centroid[3 * m + 2];
    bool bad = false;
    for (uint32_t rest = word; rest; rest &= rest - 1u) {                     // set bits in ascending order
      const int64_t i = w * 32 + (__ffs(rest) - 1);                           // < n_points: obj_word cleared the tail
      const float x = a.coords[3 * i], y = a.coords[3 * i + 1], z = a.coords[3 * i + 2];
      if (PASS == 1) {
        bad |= !(isfinite(x) && isfinite(y) && isfinite(z));
        q[0] = q[0] + static_cast<double>(x), q[1] = q[1] + static_cast<double>(y);
        q[2] = q[2] + static_cast<double>(z);
        lo[0] = x < lo[0] ? x : lo[0], lo[1] = y < lo[1] ? y : lo[1], lo[2] = z < lo[2] ? z : lo[2];
        hi[0] = x > hi[0] ? x : hi[0], hi[1] = y > hi[1] ? y : hi[1], hi[2] = z > hi[2] ? z : hi[2];
        if (a.colors != nullptr) {
          const float r = a.colors[3 * i], g = a.colors[3 * i + 1], b = a.colors[3 * i + 2];
          bad |= !(isfinite(r) && isfinite(g) && isfinite(b));
          q[3] = q[3] + static_cast<double>(r), q[4] = q[4] + static_cast<double>(g);
          q[5] = q[5] + static_cast<double>(b);
        }
      } else {
        const double dx = static_cast<double>(x) - c[0], dy = static_cast<double>(y) - c[1];
        const double dz = static_cast<double>(z) - c[2];
        q[0] = q[0] + dx * dx, q[1] = q[1] + dx * dy, q[2] = q[2] + dx * dz;
        q[3] = q[3] + dy * dy, q[4] = q[4] + dy * dz, q[5] = q[5] + dz * dz;
      }
    }
    if (bad) atomicOr(a.flags, 1);
#pragma unroll
    for (int k = 0; k < 6; ++k) q[k] = wave_tree_sum(q[k]);
    int cnt = 0;
    if (PASS == 1) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float l2 = __shfl_xor(lo[k], o, 64), h2 = __shfl_xor(hi[k], o, 64);
          lo[k] = l2 < lo[k] ? l2 : lo[k], hi[k] = h2 > hi[k] ? h2 : hi[k];
        }
      }
      cnt = wave_sum(__popc(word));
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) part[wave][k] = q[k];
      if (PASS == 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) part[wave][6 + k] = static_cast<double>(lo[k]), part[wave][9 + k] = static_cast<double>(hi[k]);
        part_cnt[wave] = cnt;
      }
    }
    __syncthreads();
    static_assert(kWaves == 2, "the waves of a chunk combine as one adjacent pair");
    if (tid < 6) out[1 + tid] = part[0][tid] + part[1][tid];
    if (PASS == 1) {
      if (tid >= 6 && tid < 9) out[1 + tid] = part[0][tid] < part[1][tid] ? part[0][tid] : part[1][tid];
      if (tid >= 9 && tid < 12) out[1 + tid] = part[0][tid] > part[1][tid] ? part[0][tid] : part[1][tid];
      if (tid == 12) out[0] = static_cast<double>(part_cnt[0] + part_cnt[1]);
    }
  }
}

// The tree over the chunks of one mask for the slab entry `q`, by one wave; every lane ends with the root.  `count`
// becomes the mask's population.
__device__ __forceinline__ double chunk_tree(const double *slab_m, int64_t chunks, int q, int lane, int64_t &count) {
  double st[kObjLevels];
  uint32_t occ = 0;
  int64_t cnt = 0;
  for (int64_t g0 = 0; g0 < chunks; g0 += 64) {                               // (wave-uniform)
    const int64_t ch = g0 + lane;
    const double n_ch = ch < chunks ? slab_m[ch * kObjSlab] : 0.0;
    double v = n_ch > 0.0 ? slab_m[ch * kObjSlab + q] : 0.0;
    cnt += static_cast<int64_t>(n_ch);
    v = wave_tree_sum(v);
    bool carry = true;
#pragma unroll
    for (int l = 0; l < kObjLevels; ++l) {
      if (carry) {
        if ((occ >> l) & 1u) {
          v = st[l] + v, occ &= ~(1u << l);
        } else {
          st[l] = v, occ |= 1u << l, carry = false;
        }
      }
    }
  }
  // what is left on the stack, padded with +0.0 (x + 0.0 == x: a partial is never -0.0)
  double acc = 0.0;
  bool has = false;
#pragma unroll
  for (int l = 0; l < kObjLevels; ++l) {
    if ((occ >> l) & 1u) acc = has ? st[l] + acc : st[l], has = true;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  count = cnt;
  return acc;
}

struct MfArgs {
  const double *slab;
  int32_t *npoint;
  double *aabb, *sum_xyz, *centroid, *cov6, *mean_color;
  int64_t chunks;
  int n, with_color;
};

// One wave per (mask, quantity).  PASS 1: quantities 0 .. 2 = the coordinate sums and the centroid, 3 = population
// and box, 4 .. 6 = colour means.  PASS 2: the six centred sums.
template <int PASS>
__global__ void __launch_bounds__(64) moments_finish_kernel(MfArgs a) {
  const int lane = threadIdx.x;
  const int nq = PASS == 1 ? (a.with_color ? 7 : 4) : 6;
  const int64_t items = static_cast<int64_t>(a.n) * nq;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {          // (wave-uniform)
    const int m = static_cast<int>(item / nq), q = static_cast<int>(item - static_cast<int64_t>(m) * nq);
    const double *slab_m = a.slab + static_cast<int64_t>(m) * a.chunks * kObjSlab;
    int64_t count = 0;
    if (PASS == 1 && q == 3) {
      double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
      for (int64_t ch = lane; ch < a.chunks; ch += 64) {
        const double n_ch = slab_m[ch * kObjSlab];
        if (n_ch > 0.0) {
          count += static_cast<int64_t>(n_ch);
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const double l2 = slab_m[ch * kObjSlab + 7 + k], h2 = slab_m[ch * kObjSlab + 10 + k];
            lo[k] = l2 < lo[k] ? l2 : lo[k], hi[k] = h2 > hi[k] ? h2 : hi[k];
          }
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        count += __shfl_xor(count, o, 64);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double l2 = __shfl_xor(lo[k], o, 64), h2 = __shfl_xor(hi[k], o, 64);
          lo[k] = l2 < lo[k] ? l2 : lo[k], hi[k] = h2 > hi[k] ? h2 : hi[k];
        }
      }
      if (lane == 0) {
        a.npoint[m] = static_cast<int32_t>(count);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          a.aabb[6 * m + k] = count ? lo[k] + 0.0 : obj_nan();
          a.aabb[6 * m + 3 + k] = count ? hi[k] + 0.0 : obj_nan();
        }
      }
      continue;
    }
    const int entry = PASS == 1 ? (q < 3 ? 1 + q : q) : 1 + q;                // (PASS 1, q = 4 .. 6: slab 4 .. 6)
    const double s = chunk_tree(slab_m, a.chunks, entry, lane, count);
    if (lane != 0) continue;
    const double mean = count ? s / static_cast<double>(count) : obj_nan();
    if (PASS == 2) {
      a.cov6[6 * m + q] = mean;
    } else if (q < 3) {
      a.sum_xyz[3 * m + q] = count ? s : obj_nan();
      a.centroid[3 * m + q] = mean;
    } else {
      a.mean_color[3 * m + (q - 4)] = mean;
    }
  }
}

// ---- extents --------------------------------------------------------------------------------------------------------
struct ExArgs {
  const uint32_t *bits;
  const float *coords;
  const double *table;                  // [A, 2] (row_stride 0) or [n, A, 2] (row_stride A): (cos, sin)
  uint64_t *keys;                       // [n, A, 4]: umin, umax, vmin, vmax as keys
  int32_t *flags;
  int64_t n_points, words, chunks;
  int n, n_angles, row_stride;
};

__global__ void __launch_bounds__(256) extents_init_kernel(uint64_t *__restrict__ keys, int64_t total) {
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll)
    keys[i] = (i & 1) ? kObjKeyMax0 : kObjKeyMin0;
}

// The chunk's mask points' (x, y) are compacted into LDS once (their order does not matter: extremes are order-free).
// A thread owns one angle and one of G = 256 / A interleaved point groups, reads the points as LDS broadcasts and
// keeps its four running extremes in registers; the groups combine through LDS; one atomic per (angle, extreme).
__global__ void __launch_bounds__(kObjExtBlock) extents_chunk_kernel(ExArgs a) {
  __shared__ float2 xy[kObjChunkWords * 32];
  __shared__ uint64_t red[kObjExtBlock * 4];
  __shared__ int fill;
  const int tid = threadIdx.x;
  const int n_ang = a.n_angles;                                               // 1 .. 180 (checked by the entry)
  const int groups = kObjExtBlock / n_ang;                                    // >= 1
  const int grp = tid / n_ang, ang = tid - grp * n_ang;
  const int64_t items = static_cast<int64_t>(a.n) * a.chunks;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {          // (block-uniform)
    const int m = static_cast<int>(item / a.chunks);
    const int64_t w = (item - static_cast<int64_t>(m) * a.chunks) * kObjChunkWords + tid;
    const uint32_t word = tid < kObjChunkWords ? obj_word(a.bits, m, w, a.words, a.n_points) : 0u;
    if (tid == 0) fill = 0;
    if (!__syncthreads_or(word != 0u)) continue;
    if (word) {
      int off = atomicAdd(&fill, __popc(word));                               // off + popc <= 32 * kObjChunkWords
      bool bad = false;
      for (uint32_t rest = word; rest; rest &= rest - 1u) {
        const int64_t i = w * 32 + (__ffs(rest) - 1);                         // < n_points
        const float x = a.coords[3 * i], y = a.coords[3 * i + 1];
        bad |= !(isfinite(x) && isfinite(y));
        xy[off++] = make_float2(x, y);
      }
      if (bad) atomicOr(a.flags, 1);
    }
    __syncthreads();
    const int total = fill;
    if (grp < groups) {
      const double *cs = a.table + (static_cast<int64_t>(m) * a.row_stride + ang) * 2;
      const double c = cs[0], s = cs[1];
      double ulo = INFINITY, uhi = -INFINITY, vlo = INFINITY, vhi = -INFINITY;
      for (int p = grp; p < total; p += groups) {
        const float2 pt = xy[p];
        const double x = static_cast<double>(pt.x), y = static_cast<double>(pt.y);
        const double u = x * c + y * s, v = y * c - x * s;
        ulo = u < ulo ? u : ulo, uhi = u > uhi ? u : uhi;
        vlo = v < vlo ? v : vlo, vhi = v > vhi ? v : vhi;
      }
      const bool has = grp < total;
      red[tid * 4 + 0] = has ? obj_key(ulo) : kObjKeyMin0;
      red[tid * 4 + 1] = has ? obj_key(uhi) : kObjKeyMax0;
      red[tid * 4 + 2] = has ? obj_key(vlo) : kObjKeyMin0;
      red[tid * 4 + 3] = has ? obj_key(vhi) : kObjKeyMax0;
    }
    __syncthreads();
    for (int e = tid; e < 4 * n_ang; e += kObjExtBlock) {
      const int e_ang = e >> 2, k = e & 3;
      uint64_t r = (k & 1) ? kObjKeyMax0 : kObjKeyMin0;
      for (int g = 0; g < groups; ++g) {
        const uint64_t x = red[(g * n_ang + e_ang) * 4 + k];
        r = (k & 1) ? (x > r ? x : r) : (x < r ? x : r);
      }
      unsigned long long *dst =
          reinterpret_cast<unsigned long long *>(a.keys + (static_cast<int64_t>(m) * n_ang + e_ang) * 4 + k);
      if (k & 1)
        atomicMax(dst, static_cast<unsigned long long>(r));
      else
        atomicMin(dst, static_cast<unsigned long long>(r));
    }
    __syncthreads();                                                          // before fill, xy and red are reused
  }
}

// One thread per mask: the keys of its A angles -> doubles (+ 0.0), the area of every angle, the smallest area with the
// lowest index.  With `decode` the doubles replace the keys in place (the caller's all-extremes array).
__global__ void __launch_bounds__(64) extents_select_kernel(uint64_t *__restrict__ keys, int n, int n_angles, int decode,
                                                            int32_t *__restrict__ best_index,
                                                            double *__restrict__ best_ext) {
  for (int64_t m = blockIdx.x * 64ll + threadIdx.x; m < n; m += gridDim.x * 64ll) {
    int best = -1;
    double best_area = 0.0, ext[4] = {obj_nan(), obj_nan(), obj_nan(), obj_nan()};
    for (int ang = 0; ang < n_angles; ++ang) {
      uint64_t *k = keys + (m * n_angles + ang) * 4;
      const bool empty = k[0] == kObjKeyMin0;
      double v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = empty ? obj_nan() : obj_key_decode(k[j]) + 0.0;
      if (decode) {
#pragma unroll
        for (int j = 0; j < 4; ++j) reinterpret_cast<double *>(k)[j] = v[j];
      }
      const double area = (v[1] - v[0]) * (v[3] - v[2]);
      if (!empty && (best < 0 || area < best_area)) {
        best = ang, best_area = area;
#pragma unroll
        for (int j = 0; j < 4; ++j) ext[j] = v[j];
      }
    }
    best_index[m] = best;
#pragma unroll
    for (int j = 0; j < 4; ++j) best_ext[4 * m + j] = ext[j];
  }
}

// ---- semantic vote --------------------------------------------------------------------------------------------------
struct ChArgs {
  const uint32_t *bits;
  const void *semantic;                 // int32 or int64 [n_points]
  int32_t *hist;                        // [n, n_classes], zeroed before the launch
  int64_t n_points, words, chunks;
  int n, n_classes, is_i64;
};

__global__ void __launch_bounds__(kObjSumBlock) class_hist_kernel(ChArgs a) {
  __shared__ int bins[kObjMaxClasses];
  const int tid = threadIdx.x;
  const int64_t items = static_cast<int64_t>(a.n) * a.chunks;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {          // (block-uniform)
    const int m = static_cast<int>(item / a.chunks);
    const int64_t w = (item - static_cast<int64_t>(m) * a.chunks) * kObjChunkWords + tid;
    const uint32_t word = obj_word(a.bits, m, w, a.words, a.n_points);
    for (int cl = tid; cl < kObjMaxClasses; cl += kObjSumBlock) bins[cl] = 0;
    if (!__syncthreads_or(word != 0u)) continue;
    for (uint32_t rest = word; rest; rest &= rest - 1u) {
      const int64_t i = w * 32 + (__ffs(rest) - 1);                           // < n_points
      const int64_t lab = a.is_i64 ? static_cast<const int64_t *>(a.semantic)[i]
                                   : static_cast<int64_t>(static_cast<const int32_t *>(a.semantic)[i]);
      if (lab >= 0 && lab < a.n_classes) atomicAdd(&bins[static_cast<int>(lab)], 1);
    }
    __syncthreads();
    for (int cl = tid; cl < a.n_classes; cl += kObjSumBlock) {
      if (bins[cl]) atomicAdd(&a.hist[static_cast<int64_t>(m) * a.n_classes + cl], bins[cl]);
    }
    __syncthreads();                                                          // before bins is cleared again
  }
}

__global__ void __launch_bounds__(64) class_best_kernel(const int32_t *__restrict__ hist, int n, int n_classes,
                                                        int32_t *__restrict__ label, int32_t *__restrict__ count) {
  for (int64_t m = blockIdx.x * 64ll + threadIdx.x; m < n; m += gridDim.x * 64ll) {
    int best = -1, best_c = 0;
    for (int cl = 0; cl < n_classes; ++cl) {
      const int c = hist[m * n_classes + cl];
      if (c > best_c) best = cl, best_c = c;                                  // (strict: the lowest class among equal)
    }
    label[m] = best, count[m] = best_c;
  }
}

static bool obj_range(const char *who, int n, int64_t n_points) {
  if (n < 0 || n > kObjMaxInst || n_points < 0 || n_points >= (1LL << 31)) {
    set_error("%s: %d masks over %lld points outside the supported range (<= %d, < 2^31)", who, n,
              static_cast<long long>(n_points), kObjMaxInst);
    return false;
  }
  return true;
}
static int64_t obj_chunks(int64_t n_points) {
  const int64_t words = (n_points + 31) / 32;
  return (words + kObjChunkWords - 1) / kObjChunkWords;
}

}  // namespace sg

using namespace sg;

extern "C" {

size_t sg_instance_moments_workspace_bytes(int n, int64_t n_points) {
  if (n < 0 || n_points < 0) return 0;
  return align_up(sizeof(double) * static_cast<size_t>(n) * static_cast<size_t>(obj_chunks(n_points)) * kObjSlab) + 256;
}

int sg_instance_moments(const uint32_t *bits, int n, int64_t n_points, const float *coords, const float *colors,
                        int32_t *npoint, double *aabb, double *sum_xyz, double *centroid, double *cov6,
                        double *mean_color, int32_t *flags, void *ws, size_t ws_bytes, sg_stream_t stream_) {
  if (!obj_range("sg_instance_moments", n, n_points)) return SG_ERR_UNSUPPORTED;
  SG_REQUIRE(flags != nullptr, "sg_instance_moments: null flags");
  hipStream_t stream = as_stream(stream_);
  if (hipMemsetAsync(flags, 0, sizeof(int32_t), stream) != hipSuccess) return check_launch("sg_instance_moments (memset)");
  if (n == 0) return SG_OK;
  SG_REQUIRE(npoint != nullptr && aabb != nullptr && sum_xyz != nullptr && centroid != nullptr && cov6 != nullptr &&
                 (colors == nullptr || mean_color != nullptr) && (n_points == 0 || (bits != nullptr && coords != nullptr)),
             "sg_instance_moments: null array");
  const int64_t chunks = obj_chunks(n_points);
  SG_REQUIRE(ws != nullptr && ws_bytes >= sg_instance_moments_workspace_bytes(n, n_points),
             "sg_instance_moments: workspace of %zu bytes, %zu needed", ws_bytes,
             sg_instance_moments_workspace_bytes(n, n_points));
  Workspace wsp(ws, ws_bytes);
  double *slab = wsp.take<double>(static_cast<size_t>(n) * static_cast<size_t>(chunks) * kObjSlab + 1);
  MoArgs a;
  a.bits = bits, a.coords = coords, a.colors = colors, a.centroid = centroid, a.slab = slab, a.flags = flags;
  a.n_points = n_points, a.words = (n_points + 31) / 32, a.chunks = chunks, a.n = n;
  MfArgs f;
  f.slab = slab, f.npoint = npoint, f.aabb = aabb, f.sum_xyz = sum_xyz, f.centroid = centroid, f.cov6 = cov6;
  f.mean_color = mean_color, f.chunks = chunks, f.n = n, f.with_color = colors != nullptr;
  const int grid = grid_for(static_cast<int64_t>(n) * chunks, 1, kObjMaxBlocks);
  const int fgrid = grid_for(static_cast<int64_t>(n) * 7, 1, kObjMaxBlocks);
  if (chunks) moments_chunk_kernel<1><<<grid, kObjSumBlock, 0, stream>>>(a);
  moments_finish_kernel<1><<<fgrid, 64, 0, stream>>>(f);
  if (chunks) moments_chunk_kernel<2><<<grid, kObjSumBlock, 0, stream>>>(a);
  moments_finish_kernel<2><<<fgrid, 64, 0, stream>>>(f);
  return check_launch("sg_instance_moments");
}

size_t sg_instance_extents_workspace_bytes(int n, int n_angles) {
  if (n < 0 || n_angles < 0) return 0;
  return align_up(sizeof(uint64_t) * static_cast<size_t>(n) * static_cast<size_t>(n_angles) * 4) + 256;
}

int sg_instance_extents(const uint32_t *bits, int n, int64_t n_points, const float *coords, const double *table,
                        int row_stride, int n_angles, int32_t *best_index, double *best_ext, double *all_ext,
                        int32_t *flags, void *ws, size_t ws_bytes, sg_stream_t stream_) {
  if (!obj_range("sg_instance_extents", n, n_points)) return SG_ERR_UNSUPPORTED;
  SG_REQUIRE(n_angles >= 1 && n_angles <= kObjMaxAngles && (row_stride == 0 || row_stride == n_angles),
             "sg_instance_extents: %d angles (1 .. %d), row stride %d (0 or the angle count)", n_angles, kObjMaxAngles,
             row_stride);
  SG_REQUIRE(flags != nullptr, "sg_instance_extents: null flags");
  hipStream_t stream = as_stream(stream_);
  if (hipMemsetAsync(flags, 0, sizeof(int32_t), stream) != hipSuccess) return check_launch("sg_instance_extents (memset)");
  if (n == 0) return SG_OK;
  SG_REQUIRE(table != nullptr && best_index != nullptr && best_ext != nullptr &&
                 (n_points == 0 || (bits != nullptr && coords != nullptr)),
             "sg_instance_extents: null array");
  uint64_t *keys = reinterpret_cast<uint64_t *>(all_ext);
  if (keys == nullptr) {
    SG_REQUIRE(ws != nullptr && ws_bytes >= sg_instance_extents_workspace_bytes(n, n_angles),
               "sg_instance_extents: workspace of %zu bytes, %zu needed", ws_bytes,
               sg_instance_extents_workspace_bytes(n, n_angles));
    Workspace wsp(ws, ws_bytes);
    keys = wsp.take<uint64_t>(static_cast<size_t>(n) * n_angles * 4);
  }
  const int64_t total = static_cast<int64_t>(n) * n_angles * 4;
  extents_init_kernel<<<grid_for(total, 256, kObjMaxBlocks), 256, 0, stream>>>(keys, total);
  ExArgs a;
  a.bits = bits, a.coords = coords, a.table = table, a.keys = keys, a.flags = flags;
  a.n_points = n_points, a.words = (n_points + 31) / 32, a.chunks = obj_chunks(n_points);
  a.n = n, a.n_angles = n_angles, a.row_stride = row_stride;
  if (a.chunks)
    extents_chunk_kernel<<<grid_for(static_cast<int64_t>(n) * a.chunks, 1, kObjMaxBlocks), kObjExtBlock, 0, stream>>>(a);
  extents_select_kernel<<<grid_for(n, 64, kObjMaxBlocks), 64, 0, stream>>>(keys, n, n_angles, all_ext != nullptr,
                                                                            best_index, best_ext);
  return check_launch("sg_instance_extents");
}

int sg_instance_class_hist(const uint32_t *bits, int n, int64_t n_points, const void *semantic, int is_i64,
                           int n_classes, int32_t *hist, int32_t *sem_label, int32_t *sem_count, sg_stream_t stream_) {
  if (!obj_range("sg_instance_class_hist", n, n_points)) return SG_ERR_UNSUPPORTED;
  if (n_classes < 1 || n_classes > kObjMaxClasses) {
    set_error("sg_instance_class_hist: %d classes outside the supported range (1 .. %d)", n_classes, kObjMaxClasses);
    return SG_ERR_UNSUPPORTED;
  }
  if (n == 0) return SG_OK;
  SG_REQUIRE(hist != nullptr && sem_label != nullptr && sem_count != nullptr &&
                 (n_points == 0 || (bits != nullptr && semantic != nullptr)),
             "sg_instance_class_hist: null array");
  hipStream_t stream = as_stream(stream_);
  if (hipMemsetAsync(hist, 0, sizeof(int32_t) * static_cast<size_t>(n) * n_classes, stream) != hipSuccess)
    return check_launch("sg_instance_class_hist (memset)");
  ChArgs a;
  a.bits = bits, a.semantic = semantic, a.hist = hist, a.n_points = n_points, a.words = (n_points + 31) / 32;
  a.chunks = obj_chunks(n_points), a.n = n, a.n_classes = n_classes, a.is_i64 = is_i64 != 0;
  if (a.chunks)
    class_hist_kernel<<<grid_for(static_cast<int64_t>(n) * a.chunks, 1, kObjMaxBlocks), kObjSumBlock, 0, stream>>>(a);
  class_best_kernel<<<grid_for(n, 64, kObjMaxBlocks), 64, 0, stream>>>(hist, n, n_classes, sem_label, sem_count);
  return check_launch("sg_instance_class_hist");
}

}  // extern "C"
