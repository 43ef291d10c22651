// train_data.hip -- the training-time data transform of the reference (softgroup/data/custom.py:52-194,
// data/kitti.py:78-118, data/s3dis.py:31-41) on gfx950: augmentation, the two elastic passes, crop counting,
// compaction, instance relabelling and the per-instance statistics; at test time (custom.py:162-194) the same
// kernels plus the S3DIS x4 split (s3dis.py:46-78) and KITTI's label decode (kitti.py:62-72).  Built with -ffp-contract=off: every
// float64 / float32 expression below restates the numpy / scipy arithmetic operation for operation.
//
// Reductions: the per-axis extrema go through order-preserving uint64 keys of the float64 values and
// integer atomics (exact, so any order gives the same bits); counts are integer atomics; the per-instance
// float64 sums are reduced per workgroup in a fixed tree and across workgroups in index order.  No float
// atomics anywhere: every output is bitwise repeatable.
#include "common.h"
#include "scan.h"

namespace {

constexpr int kBlock = 256;
constexpr int kCropMax = 16;            // candidates per sg_train_crop_count launch
constexpr int kIdTable = 1 << 14;       // open-addressing slots of sg_train_id_set
constexpr int kInstChunk = 2048;        // points per workgroup of the instance statistics
constexpr int64_t kEmpty = INT64_MIN;

// float64 -> uint64 key with the same order (negative: all bits flipped; non-negative: sign bit set)
__device__ __forceinline__ uint64_t dkey(double d) {
  uint64_t u = static_cast<uint64_t>(__double_as_longlong(d));
  return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}

struct Mat3 {
  double m[9];
};

// column a of np.matmul(p, m) for one float64 row p (dataAugment's product, custom.py:111)
__device__ __forceinline__ double rotate(const double (&p)[3], const Mat3 &m, int a) {
  return (p[0] * m.m[a] + p[1] * m.m[3 + a]) + p[2] * m.m[6 + a];
}

// stats[0..2] = key(max |x|), [3..5] = key(min x), [6..8] = key(max x) per axis
__global__ void stats_init_kernel(uint64_t *stats) {
  const int i = threadIdx.x;
  if (i < 9) stats[i] = (i >= 3 && i < 6) ? ~0ULL : 0ULL;
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    uint64_t w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    uint64_t w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}

// per-thread extrema of its points -> wave -> one set of integer atomics per wave (EXEC full at the call)
__device__ __forceinline__ void flush_stats(const uint64_t (&amax)[3], const uint64_t (&mn)[3],
                                            const uint64_t (&mx)[3], uint64_t *stats) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    uint64_t x = wave_max_u64(amax[a]), lo = wave_min_u64(mn[a]), hi = wave_max_u64(mx[a]);
    if (sg::lane_id() == 0) {
      atomicMax(reinterpret_cast<unsigned long long *>(stats + a), static_cast<unsigned long long>(x));
      atomicMin(reinterpret_cast<unsigned long long *>(stats + 3 + a), static_cast<unsigned long long>(lo));
      atomicMax(reinterpret_cast<unsigned long long *>(stats + 6 + a), static_cast<unsigned long long>(hi));
    }
  }
}

__device__ __forceinline__ void note(double v, int a, uint64_t (&amax)[3], uint64_t (&mn)[3], uint64_t (&mx)[3]) {
  const uint64_t k = dkey(v), ka = dkey(fabs(v));
  amax[a] = ka > amax[a] ? ka : amax[a];
  mn[a] = k < mn[a] ? k : mn[a];
  mx[a] = k > mx[a] ? k : mx[a];
}

// dataAugment's product (custom.py:110-111) and the working coordinates (custom.py:140, kitti.py:96)
__global__ void __launch_bounds__(kBlock) augment_kernel(const float *__restrict__ xyz, int64_t n, int has_scale,
                                                        float sf, Mat3 m, double work_scale, double down,
                                                        double *__restrict__ xyz_middle, double *__restrict__ work,
                                                        uint64_t *__restrict__ stats) {
  uint64_t amax[3] = {0, 0, 0}, mn[3] = {~0ULL, ~0ULL, ~0ULL}, mx[3] = {0, 0, 0};
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    double p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      float v = xyz[3 * i + a];
      if (has_scale) v = v * sf;            // float32 array * Python float stays float32 (NEP 50)
      p[a] = static_cast<double>(v);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double mid = rotate(p, m, a);
      xyz_middle[3 * i + a] = mid;
      double w = mid * work_scale;
      if (down != 1.0) w = w / down;
      work[3 * i + a] = w;
      note(w, a, amax, mn, mx);
    }
  }
  flush_stats(amax, mn, mx, stats);
}

// one pass of scipy.ndimage.convolve with the [1,1,1]/3 box along `axis` (stride `s`, extent `len`),
// mode='constant', cval=0: float64 sum in footprint order, rounded to float32.  blockIdx.y = grid.
__global__ void __launch_bounds__(kBlock) blur_pass_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                          int64_t cells, int64_t s, int len, double w) {
  const float *in = src + blockIdx.y * cells;
  float *out = dst + blockIdx.y * cells;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < cells;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int c = static_cast<int>((i / s) % len);
    const double lo = c > 0 ? static_cast<double>(in[i - s]) : 0.0;
    const double hi = c + 1 < len ? static_cast<double>(in[i + s]) : 0.0;
    double t = 0.0;
    t = t + lo * w;
    t = t + static_cast<double>(in[i]) * w;
    t = t + hi * w;
    out[i] = static_cast<float>(t);
  }
}

// scipy's find_interval_ascending on the axis linspace(-(b-1) gran, (b-1) gran, b) (integral nodes,
// spacing 2 gran exactly) -> interval index in [0, b-2] and the normalised distance
__device__ __forceinline__ int axis_index(double x, int b, double gran, double &nd, bool &oob) {
  const double g0 = -static_cast<double>(b - 1) * gran, st = 2.0 * gran;
  const double glast = static_cast<double>(b - 1) * gran;
  oob = oob || x < g0 || x > glast;
  double f = floor((x - g0) / st);
  int i = !(f >= 0.0) ? 0 : (f > static_cast<double>(b - 2) ? b - 2 : static_cast<int>(f));
  while (i < b - 2 && static_cast<double>(i + 1) * st + g0 <= x) ++i;
  while (i > 0 && static_cast<double>(i) * st + g0 > x) --i;
  const double gi = static_cast<double>(i) * st + g0, gj = static_cast<double>(i + 1) * st + g0;
  nd = (x - gi) / (gj - gi);
  return i;
}

// elastic's x + g(x) * mag (custom.py:66-74): trilinear in float64, corners in itertools.product order,
// weights multiplied in axis order (scipy 1.15 _rgi.py _evaluate_linear), 0 outside the grid
__global__ void __launch_bounds__(kBlock) elastic_kernel(double *__restrict__ x, int64_t n,
                                                        const float *__restrict__ grids, int b0, int b1, int b2,
                                                        double gran, double mag, uint64_t *__restrict__ stats) {
  uint64_t amax[3] = {0, 0, 0}, mn[3] = {~0ULL, ~0ULL, ~0ULL}, mx[3] = {0, 0, 0};
  const int64_t cells = static_cast<int64_t>(b0) * b1 * b2;
  for (int64_t p = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; p < n;
       p += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const double x0 = x[3 * p], x1 = x[3 * p + 1], x2 = x[3 * p + 2];
    bool oob = false;
    double d0, d1, d2;
    const int i0 = axis_index(x0, b0, gran, d0, oob);
    const int i1 = axis_index(x1, b1, gran, d1, oob);
    const int i2 = axis_index(x2, b2, gran, d2, oob);
    const double wa[2] = {1.0 - d0, d0}, wb[2] = {1.0 - d1, d1}, wc[2] = {1.0 - d2, d2};
    double g[3] = {0.0, 0.0, 0.0};
    if (!oob) {
      const int64_t base = (static_cast<int64_t>(i0) * b1 + i1) * b2 + i2;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int c0 = c >> 2, c1 = (c >> 1) & 1, c2 = c & 1;
        double wt = 1.0;
        wt = wt * wa[c0];
        wt = wt * wb[c1];
        wt = wt * wc[c2];
        const int64_t off = base + (static_cast<int64_t>(c0) * b1 + c1) * b2 + c2;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          g[k] = g[k] + static_cast<double>(grids[k * cells + off]) * wt;
        }
      }
    }
    const double xn[3] = {x0 + g[0] * mag, x1 + g[1] * mag, x2 + g[2] * mag};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      x[3 * p + a] = xn[a];
      note(xn[a], a, amax, mn, mx);
    }
  }
  flush_stats(amax, mn, mx, stats);
}

struct Crops {
  double v[kCropMax][6];     // offset x y z, spatial shape x y z
};

// the shifted working coordinate of custom.py:143 (kitti.py:101-103): (x * down) - min
__device__ __forceinline__ double shifted(double x, double down, double mn) {
  return (down != 1.0 ? x * down : x) - mn;
}

__device__ __forceinline__ bool inside(const double (&t)[3], const double *c) {
  const double o0 = t[0] + c[0], o1 = t[1] + c[1], o2 = t[2] + c[2];
  return fmin(fmin(o0, o1), o2) >= 0.0 && o0 < c[3] && o1 < c[4] && o2 < c[5];
}

__global__ void __launch_bounds__(kBlock) crop_count_kernel(const double *__restrict__ x, int64_t n, double down,
                                                           double m0, double m1, double m2, Crops cr, int k,
                                                           unsigned long long *__restrict__ counts) {
  int cnt[kCropMax];
#pragma unroll
  for (int j = 0; j < kCropMax; ++j) cnt[j] = 0;
  for (int64_t p = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; p < n;
       p += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const double t[3] = {shifted(x[3 * p], down, m0), shifted(x[3 * p + 1], down, m1),
                         shifted(x[3 * p + 2], down, m2)};
#pragma unroll
    for (int j = 0; j < kCropMax; ++j)
      if (j < k && inside(t, cr.v[j])) ++cnt[j];
  }
#pragma unroll
  for (int j = 0; j < kCropMax; ++j) {
    if (j < k) {                       // (k is uniform: EXEC stays full for the DPP sum)
      const int s = sg::wave_sum(cnt[j]);
      if (sg::lane_id() == 0 && s) atomicAdd(counts + j, static_cast<unsigned long long>(s));
    }
  }
}

struct CompactIn {
  const double *x;
  double down, m0, m1, m2;
  int has_crop;
  double crop[6];
  __device__ __forceinline__ void t(int64_t i, double (&o)[3]) const {
    o[0] = shifted(x[3 * i], down, m0);
    o[1] = shifted(x[3 * i + 1], down, m1);
    o[2] = shifted(x[3 * i + 2], down, m2);
  }
  __device__ __forceinline__ int operator()(int64_t i) const {
    if (!has_crop) return 1;
    double o[3];
    t(i, o);
    return inside(o, crop) ? 1 : 0;
  }
};

struct CompactOut {
  CompactIn in;
  const double *xyz_middle;
  const float *feat, *noise;
  int c;
  const int64_t *sem, *inst;
  int64_t *coord;
  double *mid_out;
  float *feat_out;
  int64_t *sem_out, *inst_out;
  int64_t cap;
  __device__ __forceinline__ void operator()(int64_t i, int r) const {
    if (r >= cap) return;              // (the caller sized the outputs from the same test's count)
    double o[3];
    in.t(i, o);
    if (in.has_crop) {
      if (!inside(o, in.crop)) return;
      o[0] = o[0] + in.crop[0];
      o[1] = o[1] + in.crop[1];
      o[2] = o[2] + in.crop[2];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      coord[3 * static_cast<int64_t>(r) + a] = static_cast<int64_t>(o[a]);      // torch .long(): trunc
      mid_out[3 * static_cast<int64_t>(r) + a] = xyz_middle[3 * i + a];
    }
    for (int j = 0; j < c; ++j) {
      float f = feat[i * c + j];
      if (noise) f = f + noise[j];
      feat_out[static_cast<int64_t>(r) * c + j] = f;
    }
    sem_out[r] = sem[i];
    inst_out[r] = inst[i];
  }
};

__global__ void __launch_bounds__(kBlock) gather_kernel(const int64_t *__restrict__ idx, int64_t m,
                                                       const float *__restrict__ xyz, const float *__restrict__ feat,
                                                       int c, const int64_t *__restrict__ sem,
                                                       const int64_t *__restrict__ inst, float *__restrict__ xyz_out,
                                                       float *__restrict__ feat_out, int64_t *__restrict__ sem_out,
                                                       int64_t *__restrict__ inst_out) {
  for (int64_t r = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; r < m;
       r += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t i = idx[r];
    for (int a = 0; a < 3; ++a) xyz_out[3 * r + a] = xyz[3 * i + a];
    for (int j = 0; j < c; ++j) feat_out[r * c + j] = feat[i * c + j];
    sem_out[r] = sem[i];
    inst_out[r] = inst[i];
  }
}

__global__ void __launch_bounds__(kBlock) id_table_init_kernel(int64_t *table, int64_t *out) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < kIdTable; i += gridDim.x * blockDim.x) table[i] = kEmpty;
  if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = 0;
}

// the set of labels != ignore: CAS-inserted into an open-addressing table; new ids appended to out[1..]
// (in no particular order: the caller sorts the set), their number in out[0]
__global__ void __launch_bounds__(kBlock) id_set_kernel(const int64_t *__restrict__ lab, int64_t n, int64_t ignore,
                                                       int64_t *__restrict__ table, int64_t *__restrict__ out,
                                                       int cap) {
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t v = lab[i];
    if (v == ignore) continue;
    uint32_t slot = static_cast<uint32_t>(sg::mix64(static_cast<uint64_t>(v))) & (kIdTable - 1);
    for (int probe = 0; probe < kIdTable; ++probe) {
      int64_t cur = __hip_atomic_load(table + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == v) break;
      if (cur == kEmpty) {
        cur = static_cast<int64_t>(atomicCAS(reinterpret_cast<unsigned long long *>(table + slot),
                                             static_cast<unsigned long long>(kEmpty),
                                             static_cast<unsigned long long>(v)));
        if (cur == kEmpty) {
          const unsigned long long r = atomicAdd(reinterpret_cast<unsigned long long *>(out), 1ULL);
          if (r < static_cast<unsigned long long>(cap)) out[1 + r] = v;
          break;
        }
        if (cur == v) break;
      }
      slot = (slot + 1) & (kIdTable - 1);
    }
  }
}

// labels found in sorted_ids[0..k) -> mapped[...]; the rest (the ignore label) unchanged
__global__ void __launch_bounds__(kBlock) remap_kernel(int64_t *__restrict__ lab, int64_t n,
                                                      const int64_t *__restrict__ sorted_ids,
                                                      const int64_t *__restrict__ mapped, int k) {
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t v = lab[i];
    int lo = 0, hi = k;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (sorted_ids[mid] < v) lo = mid + 1; else hi = mid;
    }
    if (lo < k && sorted_ids[lo] == v) lab[i] = mapped[lo];
  }
}

struct InstSlab {
  double s[3];
  int64_t count, first;
};

// grid (chunks, instances): the points of chunk blockIdx.x with label blockIdx.y -> count, first index,
// float64 sum of xyz_middle (per thread over its contiguous points in order, then a fixed LDS tree)
__global__ void __launch_bounds__(kBlock) inst_partial_kernel(const double *__restrict__ mid,
                                                             const int64_t *__restrict__ lab, int64_t n,
                                                             InstSlab *__restrict__ slab, int n_chunks) {
  __shared__ double ls[3][kBlock];
  __shared__ int64_t lc[kBlock], lf[kBlock];
  const int inst = blockIdx.y;
  constexpr int per = kInstChunk / kBlock;
  const int64_t first = static_cast<int64_t>(blockIdx.x) * kInstChunk + threadIdx.x * per;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  int64_t c = 0, f = INT64_MAX;
#pragma unroll
  for (int j = 0; j < per; ++j) {
    const int64_t i = first + j;
    if (i < n && lab[i] == inst) {
      s0 = s0 + mid[3 * i];
      s1 = s1 + mid[3 * i + 1];
      s2 = s2 + mid[3 * i + 2];
      if (c == 0) f = i;
      ++c;
    }
  }
  ls[0][threadIdx.x] = s0;
  ls[1][threadIdx.x] = s1;
  ls[2][threadIdx.x] = s2;
  lc[threadIdx.x] = c;
  lf[threadIdx.x] = f;
  __syncthreads();
  for (int h = kBlock / 2; h > 0; h >>= 1) {
    if (threadIdx.x < h) {
      const int o = threadIdx.x + h;
      ls[0][threadIdx.x] = ls[0][threadIdx.x] + ls[0][o];
      ls[1][threadIdx.x] = ls[1][threadIdx.x] + ls[1][o];
      ls[2][threadIdx.x] = ls[2][threadIdx.x] + ls[2][o];
      lc[threadIdx.x] += lc[o];
      lf[threadIdx.x] = lf[o] < lf[threadIdx.x] ? lf[o] : lf[threadIdx.x];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    InstSlab &r = slab[static_cast<int64_t>(inst) * n_chunks + blockIdx.x];
    r.s[0] = ls[0][0];
    r.s[1] = ls[1][0];
    r.s[2] = ls[2][0];
    r.count = lc[0];
    r.first = lf[0];
  }
}

// one thread per instance: the chunks' partials in chunk order -> point count, class of the first point
// (shifted unless -100), mean rounded to float32 (getInstanceInfo, custom.py:81-88)
__global__ void __launch_bounds__(64) inst_final_kernel(const InstSlab *__restrict__ slab, int n_chunks, int k,
                                                       const int64_t *__restrict__ sem, int64_t cls_shift,
                                                       int32_t *__restrict__ pointnum, int64_t *__restrict__ cls,
                                                       float *__restrict__ mean) {
  const int inst = blockIdx.x * blockDim.x + threadIdx.x;
  if (inst >= k) return;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  int64_t c = 0, f = INT64_MAX;
  for (int j = 0; j < n_chunks; ++j) {
    const InstSlab &r = slab[static_cast<int64_t>(inst) * n_chunks + j];
    s0 = s0 + r.s[0];
    s1 = s1 + r.s[1];
    s2 = s2 + r.s[2];
    c += r.count;
    f = r.first < f ? r.first : f;
  }
  pointnum[inst] = static_cast<int32_t>(c);
  const int64_t sc = c ? sem[f] : -100;
  cls[inst] = sc != -100 ? sc - cls_shift : sc;
  const double dc = static_cast<double>(c);
  mean[3 * inst] = static_cast<float>(s0 / dc);
  mean[3 * inst + 1] = static_cast<float>(s1 / dc);
  mean[3 * inst + 2] = static_cast<float>(s2 / dc);
}

// pt_offset_label = float32 mean (or -100) - float64 point (custom.py:76-89)
__global__ void __launch_bounds__(kBlock) inst_offset_kernel(const double *__restrict__ mid,
                                                            const int64_t *__restrict__ lab, int64_t n, int k,
                                                            const float *__restrict__ mean,
                                                            double *__restrict__ off) {
  for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t l = lab[i];
    const int32_t l32 = static_cast<int32_t>(l);      // (getInstanceInfo reads instance_label.astype(np.int32))
    const bool in = l32 >= 0 && l32 < k;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float m = in ? mean[3 * l32 + a] : -100.0f;
      off[3 * i + a] = static_cast<double>(m) - mid[3 * i + a];
    }
  }
}

// ---- test time: transform_test's S3DIS x4 split (s3dis.py:46-78) and KITTI's label decode (kitti.py:62-72) ----
// One thread per quad of consecutive points 4g .. 4g+3 (point i belongs to piece i % 4).

// the quad's rows of a float32 [n, 3] array: three 16-byte loads when all four rows exist and `vec` (the array
// 16-byte aligned); returns how many of the four rows exist
__device__ __forceinline__ int load_quad(const float *__restrict__ v, int64_t n, int64_t g, bool vec,
                                         float (&p)[12]) {
  const int64_t i0 = 4 * g;
  const int cnt = n - i0 >= 4 ? 4 : static_cast<int>(n - i0);
  if (cnt == 4 && vec) {
    const float4 *q = reinterpret_cast<const float4 *>(v + 3 * i0);
    const float4 a = q[0], b = q[1], c = q[2];
    p[0] = a.x, p[1] = a.y, p[2] = a.z, p[3] = a.w;
    p[4] = b.x, p[5] = b.y, p[6] = b.z, p[7] = b.w;
    p[8] = c.x, p[9] = c.y, p[10] = c.z, p[11] = c.w;
  } else {
#pragma unroll
    for (int j = 0; j < 12; ++j) p[j] = j < 3 * cnt ? v[3 * i0 + j] : 0.0f;
  }
  return cnt;
}

// the quad's int64 labels: two 16-byte loads when all four exist and `vec`
__device__ __forceinline__ void load_quad_i64(const int64_t *__restrict__ v, int64_t g, int cnt, bool vec,
                                              int64_t (&p)[4]) {
  if (cnt == 4 && vec) {
    const longlong2 *q = reinterpret_cast<const longlong2 *>(v + 4 * g);
    const longlong2 a = q[0], b = q[1];
    p[0] = a.x, p[1] = a.y, p[2] = b.x, p[3] = b.y;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = j < cnt ? v[4 * g + j] : 0;
  }
}

__global__ void x4_stats_init_kernel(uint64_t *stats) {
  const int i = threadIdx.x;
  if (i < 13) stats[i] = i < 12 ? ~0ULL : 0ULL;
}

// pass 1: key(min of xyz_middle * scale) per piece b and axis a -> stats[3 b + a]; stats[12] = 1 when a value
// is not finite (the caller then leaves the scan to the host)
__global__ void __launch_bounds__(kBlock) x4_minima_kernel(const float *__restrict__ xyz, int64_t n, bool vec,
                                                          Mat3 m, double scale, uint64_t *__restrict__ stats) {
  uint64_t mn[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) mn[j] = ~0ULL;
  bool bad = false;
  const int64_t quads = (n + 3) / 4;
  for (int64_t g = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; g < quads;
       g += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    float f[12];
    const int cnt = load_quad(xyz, n, g, vec, f);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      if (b < cnt) {
        const double p[3] = {f[3 * b], f[3 * b + 1], f[3 * b + 2]};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const double w = rotate(p, m, a) * scale;
          bad = bad || !isfinite(w);
          const uint64_t k = dkey(w);
          mn[3 * b + a] = k < mn[3 * b + a] ? k : mn[3 * b + a];
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 12; ++j) {
    const uint64_t lo = wave_min_u64(mn[j]);
    if (sg::lane_id() == 0 && lo != ~0ULL)
      atomicMin(reinterpret_cast<unsigned long long *>(stats + j), static_cast<unsigned long long>(lo));
  }
  const uint64_t flag = wave_max_u64(bad ? 1ULL : 0ULL);
  if (sg::lane_id() == 0 && flag) atomicMax(reinterpret_cast<unsigned long long *>(stats + 12), 1ULL);
}

struct X4Pieces {
  double mn[12];          // per piece and axis: min of xyz_middle * scale
  int64_t start[4];       // first output row of each piece
};

// pass 2: point 4g + b -> row start[b] + g: coord [b, trunc(xyz_middle * scale - min_b)] (int64 [n, 4]),
// xyz_middle, feat, labels -- the reference's concatenation order (s3dis.py:62-75)
__global__ void __launch_bounds__(kBlock) x4_split_kernel(const float *__restrict__ xyz,
                                                         const float *__restrict__ feat, int c,
                                                         const int64_t *__restrict__ sem,
                                                         const int64_t *__restrict__ inst, int64_t n, bool vec,
                                                         Mat3 m, double scale, X4Pieces pc,
                                                         int64_t *__restrict__ coord, double *__restrict__ mid,
                                                         float *__restrict__ feat_out, int64_t *__restrict__ sem_out,
                                                         int64_t *__restrict__ inst_out) {
  const int64_t quads = (n + 3) / 4;
  for (int64_t g = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; g < quads;
       g += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    float f[12], fe[12];
    int64_t ls[4], li[4];
    const int cnt = load_quad(xyz, n, g, vec, f);
    const bool feat3 = c == 3 && cnt == 4 && vec;
    if (feat3) load_quad(feat, n, g, true, fe);
    load_quad_i64(sem, g, cnt, vec, ls);
    load_quad_i64(inst, g, cnt, vec, li);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      if (b >= cnt) continue;
      const int64_t r = pc.start[b] + g;
      const double p[3] = {f[3 * b], f[3 * b + 1], f[3 * b + 2]};
      double w[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double md = rotate(p, m, a);
        mid[3 * r + a] = md;
        w[a] = md * scale - pc.mn[3 * b + a];
      }
      longlong2 *crow = reinterpret_cast<longlong2 *>(coord + 4 * r);
      crow[0] = make_longlong2(b, static_cast<int64_t>(w[0]));       // torch .long(): trunc
      crow[1] = make_longlong2(static_cast<int64_t>(w[1]), static_cast<int64_t>(w[2]));
      if (feat3) {
#pragma unroll
        for (int j = 0; j < 3; ++j) feat_out[3 * r + j] = fe[3 * b + j];
      } else {
        for (int j = 0; j < c; ++j) feat_out[r * c + j] = feat[(4 * g + b) * c + j];
      }
      sem_out[r] = ls[b];
      inst_out[r] = li[b];
    }
  }
}

constexpr int32_t kNoKey = INT32_MIN;     // learning-map table entry of a key the map lacks

// sem = lut[word & 0xFFFF] (-100 for a missing key), inst = word where sem > 10 else -100; *missing = smallest
// index whose key is missing (left at all ones when none is)
__global__ void __launch_bounds__(kBlock) kitti_decode_kernel(const int32_t *__restrict__ words, int64_t n, bool vec,
                                                             const int32_t *__restrict__ lut,
                                                             int64_t *__restrict__ sem, int64_t *__restrict__ inst,
                                                             uint64_t *__restrict__ missing) {
  uint64_t first = ~0ULL;
  const int64_t quads = (n + 3) / 4;
  for (int64_t g = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; g < quads;
       g += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t i0 = 4 * g;
    const int cnt = n - i0 >= 4 ? 4 : static_cast<int>(n - i0);
    int32_t w[4];
    if (cnt == 4 && vec) {
      const int4 q = *reinterpret_cast<const int4 *>(words + i0);
      w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b) w[b] = b < cnt ? words[i0 + b] : 0;
    }
    int64_t s[4], t[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int32_t l = lut[w[b] & 0xFFFF];
      if (l == kNoKey && b < cnt && first == ~0ULL) first = static_cast<uint64_t>(i0 + b);
      s[b] = l == kNoKey ? -100 : l;
      t[b] = l != kNoKey && l > 10 ? w[b] : -100;
    }
    if (cnt == 4 && vec) {
      longlong2 *ps = reinterpret_cast<longlong2 *>(sem + i0), *pt = reinterpret_cast<longlong2 *>(inst + i0);
      ps[0] = make_longlong2(s[0], s[1]);
      ps[1] = make_longlong2(s[2], s[3]);
      pt[0] = make_longlong2(t[0], t[1]);
      pt[1] = make_longlong2(t[2], t[3]);
    } else {
      for (int b = 0; b < cnt; ++b) {
        sem[i0 + b] = s[b];
        inst[i0 + b] = t[b];
      }
    }
  }
  const uint64_t lo = wave_min_u64(first);
  if (sg::lane_id() == 0 && lo != ~0ULL)
    atomicMin(reinterpret_cast<unsigned long long *>(missing), static_cast<unsigned long long>(lo));
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline int blocks_for(int64_t n) { return sg::grid_for(n, kBlock, 1024); }

}  // namespace

extern "C" {

int sg_train_augment(const float *xyz, int64_t n, int has_scale, float scale_factor, const double *m_host,
                     double work_scale, double down, double *xyz_middle, double *work, uint64_t *stats,
                     sg_stream_t stream) {
  SG_REQUIRE(n >= 0 && m_host && stats && (n == 0 || (xyz && xyz_middle && work)) && down > 0,
             "sg_train_augment: bad arguments");
  hipStream_t s = sg::as_stream(stream);
  Mat3 m;
  for (int i = 0; i < 9; ++i) m.m[i] = m_host[i];
  stats_init_kernel<<<1, 64, 0, s>>>(stats);
  if (n) augment_kernel<<<blocks_for(n), kBlock, 0, s>>>(xyz, n, has_scale, scale_factor, m, work_scale, down,
                                                          xyz_middle, work, stats);
  return sg::check_launch("sg_train_augment");
}

int sg_train_blur(float *grids, float *tmp, int b0, int b1, int b2, int n_grids, sg_stream_t stream) {
  SG_REQUIRE(grids && tmp && b0 > 0 && b1 > 0 && b2 > 0 && n_grids > 0 && n_grids <= 65535,
             "sg_train_blur: bad arguments");
  hipStream_t s = sg::as_stream(stream);
  const int64_t cells = static_cast<int64_t>(b0) * b1 * b2;
  const int64_t stride[3] = {static_cast<int64_t>(b1) * b2, b2, 1};
  const int len[3] = {b0, b1, b2};
  const double w = static_cast<double>(1.0f / 3.0f);       // np.ones(..).astype('float32') / 3
  dim3 grid(blocks_for(cells), n_grids);
  float *src = grids, *dst = tmp;
  for (int pass = 0; pass < 6; ++pass) {                   // x, y, z, x, y, z (custom.py:59-64)
    const int a = pass % 3;
    blur_pass_kernel<<<grid, kBlock, 0, s>>>(src, dst, cells, stride[a], len[a], w);
    float *t = src;
    src = dst;
    dst = t;
  }
  return sg::check_launch("sg_train_blur");                // (six passes: the result is back in `grids`)
}

int sg_train_elastic(double *work, int64_t n, const float *grids, int b0, int b1, int b2, double gran, double mag,
                     uint64_t *stats, sg_stream_t stream) {
  SG_REQUIRE(n >= 0 && stats && (n == 0 || (work && grids)) && b0 >= 2 && b1 >= 2 && b2 >= 2 && gran > 0,
             "sg_train_elastic: bad arguments");
  hipStream_t s = sg::as_stream(stream);
  stats_init_kernel<<<1, 64, 0, s>>>(stats);
  if (n) elastic_kernel<<<blocks_for(n), kBlock, 0, s>>>(work, n, grids, b0, b1, b2, gran, mag, stats);
  return sg::check_launch("sg_train_elastic");
}

int sg_train_crop_count(const double *work, int64_t n, double down, const double *min_host,
                        const double *cand_host, int k, uint64_t *counts, sg_stream_t stream) {
  SG_REQUIRE(n >= 0 && min_host && cand_host && counts && k >= 1 && k <= kCropMax && (n == 0 || work) && down > 0,
             "sg_train_crop_count: bad arguments (1 <= k <= %d)", kCropMax);
  hipStream_t s = sg::as_stream(stream);
  Crops cr;
  for (int j = 0; j < kCropMax; ++j)
    for (int a = 0; a < 6; ++a) cr.v[j][a] = j < k ? cand_host[6 * j + a] : 0.0;
  hipMemsetAsync(counts, 0, sizeof(uint64_t) * k, s);
  if (n)
    crop_count_kernel<<<blocks_for(n), kBlock, 0, s>>>(work, n, down, min_host[0], min_host[1], min_host[2], cr, k,
                                                       reinterpret_cast<unsigned long long *>(counts));
  return sg::check_launch("sg_train_crop_count");
}

size_t sg_train_compact_workspace_bytes(int64_t n) { return sg::scan_workspace_bytes(n); }

int sg_train_compact(const double *work, const double *xyz_middle, const float *feat, int c, const float *noise,
                     const int64_t *sem, const int64_t *inst, int64_t n, double down, const double *min_host,
                     const double *crop_host, int64_t out_cap, int64_t *coord, double *xyz_middle_out,
                     float *feat_out, int64_t *sem_out, int64_t *inst_out, int32_t *kept, void *ws,
                     size_t ws_bytes, sg_stream_t stream) {
  SG_REQUIRE(n >= 0 && c >= 0 && min_host && kept && down > 0 &&
                 (n == 0 || (work && xyz_middle && (feat || c == 0) && sem && inst && coord && xyz_middle_out &&
                             (feat_out || c == 0) && sem_out && inst_out)),
             "sg_train_compact: bad arguments");
  CompactIn in{work, down, min_host[0], min_host[1], min_host[2], crop_host != nullptr, {0, 0, 0, 0, 0, 0}};
  if (crop_host)
    for (int a = 0; a < 6; ++a) in.crop[a] = crop_host[a];
  CompactOut out{in, xyz_middle, feat, noise, c, sem, inst, coord, xyz_middle_out, feat_out, sem_out, inst_out,
                 out_cap};
  return sg::exclusive_scan(in, out, n, kept, ws, ws_bytes, sg::as_stream(stream));
}

int sg_train_gather(const int64_t *idx, int64_t m, const float *xyz, const float *feat, int c, const int64_t *sem,
                    const int64_t *inst, float *xyz_out, float *feat_out, int64_t *sem_out, int64_t *inst_out,
                    sg_stream_t stream) {
  SG_REQUIRE(m >= 0 && c >= 0 &&
                 (m == 0 || (idx && xyz && sem && inst && xyz_out && sem_out && inst_out &&
                             (c == 0 || (feat && feat_out)))),
             "sg_train_gather: bad arguments");
  if (m)
    gather_kernel<<<blocks_for(m), kBlock, 0, sg::as_stream(stream)>>>(idx, m, xyz, feat, c, sem, inst, xyz_out,
                                                                       feat_out, sem_out, inst_out);
  return sg::check_launch("sg_train_gather");
}

size_t sg_train_id_set_workspace_bytes(void) { return sg::align_up(sizeof(int64_t) * kIdTable); }

int sg_train_id_set(const int64_t *labels, int64_t n, int64_t ignore, int64_t *out, int cap, void *ws,
                    size_t ws_bytes, sg_stream_t stream) {
  SG_REQUIRE(n >= 0 && out && cap >= 0 && cap <= kIdTable / 2 && (n == 0 || labels),
             "sg_train_id_set: bad arguments (cap <= %d)", kIdTable / 2);
  SG_REQUIRE(ws && ws_bytes >= sg_train_id_set_workspace_bytes(), "sg_train_id_set: workspace too small");
  hipStream_t s = sg::as_stream(stream);
  int64_t *table = static_cast<int64_t *>(ws);
  id_table_init_kernel<<<kIdTable / kBlock, kBlock, 0, s>>>(table, out);
  if (n) id_set_kernel<<<blocks_for(n), kBlock, 0, s>>>(labels, n, ignore, table, out, cap);
  return sg::check_launch("sg_train_id_set");
}

int sg_train_remap(int64_t *labels, int64_t n, const int64_t *sorted_ids, const int64_t *mapped, int k,
                   sg_stream_t stream) {
  SG_REQUIRE(n >= 0 && k >= 0 && (n == 0 || labels) && (k == 0 || (sorted_ids && mapped)),
             "sg_train_remap: bad arguments");
  if (n && k) remap_kernel<<<blocks_for(n), kBlock, 0, sg::as_stream(stream)>>>(labels, n, sorted_ids, mapped, k);
  return sg::check_launch("sg_train_remap");
}

size_t sg_train_instance_workspace_bytes(int64_t n, int k) {
  const int64_t chunks = (n + kInstChunk - 1) / kInstChunk;
  return sg::align_up(sizeof(InstSlab) * static_cast<size_t>(chunks > 0 ? chunks : 1) * (k > 0 ? k : 1)) +
         sg::align_up(sizeof(float) * 3 * (k > 0 ? k : 1));
}

int sg_train_instance_info(const double *xyz_middle, const int64_t *inst, const int64_t *sem, int64_t n, int k,
                           int64_t cls_shift, int32_t *pointnum, int64_t *cls, double *pt_offset, void *ws,
                           size_t ws_bytes, sg_stream_t stream) {
  SG_REQUIRE(n >= 0 && k >= 0 && k <= 65535 && (n == 0 || (xyz_middle && inst && sem && pt_offset)) &&
                 (k == 0 || (pointnum && cls)),
             "sg_train_instance_info: bad arguments (k <= 65535)");
  SG_REQUIRE(ws && ws_bytes >= sg_train_instance_workspace_bytes(n, k), "sg_train_instance_info: workspace too small");
  hipStream_t s = sg::as_stream(stream);
  const int chunks = static_cast<int>((n + kInstChunk - 1) / kInstChunk);
  sg::Workspace w(ws, ws_bytes);
  InstSlab *slab = w.take<InstSlab>(static_cast<size_t>(chunks > 0 ? chunks : 1) * (k > 0 ? k : 1));
  float *mean = w.take<float>(3 * (k > 0 ? k : 1));
  if (k && chunks) {
    inst_partial_kernel<<<dim3(chunks, k), kBlock, 0, s>>>(xyz_middle, inst, n, slab, chunks);
    inst_final_kernel<<<(k + 63) / 64, 64, 0, s>>>(slab, chunks, k, sem, cls_shift, pointnum, cls, mean);
  }
  if (n) inst_offset_kernel<<<blocks_for(n), kBlock, 0, s>>>(xyz_middle, inst, n, k, mean, pt_offset);
  return sg::check_launch("sg_train_instance_info");
}

int sg_test_x4_minima(const float *xyz, int64_t n, const double *m_host, double scale, uint64_t *stats,
                      sg_stream_t stream) {
  SG_REQUIRE(n >= 0 && m_host && stats && (n == 0 || xyz), "sg_test_x4_minima: bad arguments");
  hipStream_t s = sg::as_stream(stream);
  Mat3 m;
  for (int i = 0; i < 9; ++i) m.m[i] = m_host[i];
  x4_stats_init_kernel<<<1, 64, 0, s>>>(stats);
  if (n)
    x4_minima_kernel<<<blocks_for((n + 3) / 4), kBlock, 0, s>>>(xyz, n, aligned16(xyz), m, scale, stats);
  return sg::check_launch("sg_test_x4_minima");
}

int sg_test_x4_split(const float *xyz, const float *feat, int c, const int64_t *sem, const int64_t *inst, int64_t n,
                     const double *m_host, double scale, const double *min_host, int64_t *coord,
                     double *xyz_middle, float *feat_out, int64_t *sem_out, int64_t *inst_out, sg_stream_t stream) {
  SG_REQUIRE(n >= 0 && c >= 0 && m_host && min_host &&
                 (n == 0 || (xyz && sem && inst && coord && xyz_middle && sem_out && inst_out &&
                             (c == 0 || (feat && feat_out)))),
             "sg_test_x4_split: bad arguments");
  SG_REQUIRE(aligned16(coord), "sg_test_x4_split: coord must be 16-byte aligned");
  X4Pieces pc;
  Mat3 m;
  for (int i = 0; i < 9; ++i) m.m[i] = m_host[i];
  for (int i = 0; i < 12; ++i) pc.mn[i] = min_host[i];
  int64_t row = 0;
  for (int b = 0; b < 4; ++b) {            // piece b holds points b, b + 4, ...: ceil((n - b) / 4) of them
    pc.start[b] = row;
    row += n > b ? (n - b + 3) / 4 : 0;
  }
  const bool vec = aligned16(xyz) && aligned16(sem) && aligned16(inst) && (c == 0 || aligned16(feat));
  if (n)
    x4_split_kernel<<<blocks_for((n + 3) / 4), kBlock, 0, sg::as_stream(stream)>>>(
        xyz, feat, c, sem, inst, n, vec, m, scale, pc, coord, xyz_middle, feat_out, sem_out, inst_out);
  return sg::check_launch("sg_test_x4_split");
}

int sg_kitti_decode_labels(const int32_t *words, int64_t n, const int32_t *lut, int64_t *sem, int64_t *inst,
                           uint64_t *missing, sg_stream_t stream) {
  SG_REQUIRE(n >= 0 && lut && missing && (n == 0 || (words && sem && inst)), "sg_kitti_decode_labels: bad arguments");
  hipStream_t s = sg::as_stream(stream);
  hipMemsetAsync(missing, 0xFF, sizeof(uint64_t), s);
  const bool vec = aligned16(words) && aligned16(sem) && aligned16(inst);
  if (n) kitti_decode_kernel<<<blocks_for((n + 3) / 4), kBlock, 0, s>>>(words, n, vec, lut, sem, inst, missing);
  return sg::check_launch("sg_kitti_decode_labels");
}

}  // extern "C"
