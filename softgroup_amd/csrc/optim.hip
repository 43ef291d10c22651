// optim.hip -- the optimizer step of the training loop as multi-tensor kernels: gradient norm + clip
// coefficient (torch.nn.utils.clip_grad_norm_), AMP unscale / skip (torch.amp.GradScaler) and the Adam / AdamW /
// SGD update of torch.optim, one launch per parameter group instead of ~30 foreach passes.
//
// The model has a few hundred small parameter tensors: the cost of the torch form is launches and host work, not
// bytes.  Here a device table holds one column per tensor (addresses of param, grad, two states, the step
// counter; the element count) and a second table cuts the tensors into chunks of kOptChunk elements; workgroups
// walk the chunk table.  Nothing depends on the number of tensors: no per-launch limit, no argument packing.
//
// Arithmetic: every element is read as float32, the update is evaluated in double and each stored quantity is
// rounded once (the scheme of the mask loss in losses.hip).  That is the float64 form of torch's single-tensor
// formulas to half an ulp, whichever way a float32 build contracts them.
//
// Sums (the norm): per-thread double accumulation, fixed xor butterfly across the wave, wave order in LDS,
// per-workgroup partials added by ONE workgroup of a second launch.  No float atomics, no arrival counters:
// two runs give the same bits.
//
// The step counter is torch's float32 device scalar (capturable layout), read by every chunk of its tensor and
// advanced once.  For a tensor of several chunks the last chunk to finish advances it (an INTEGER counter per
// tensor that the same workgroup puts back to zero), so no chunk can read the advanced value.
#include "common.h"

namespace sg {

constexpr int kOptBlock = 256;
constexpr int kOptQuads = 8;                                   // float4 per thread and chunk
constexpr int kOptChunk = kOptBlock * kOptQuads * 4;           // 8192 elements
constexpr int kOptFlight = 4;                                  // float4 loads in flight per thread and array
constexpr int kOptMaxBlocks = 2048;                            // step / scale launches
constexpr int kOptNormBlocks = 1024;                           // norm partials

static size_t optim_ws_bytes() { return align_up(sizeof(double) * 2 * kOptNormBlocks); }

struct Chunk {
  int t;            // tensor
  int n;            // elements of this chunk
  int64_t off;      // first element
  int64_t count;    // elements of the tensor
};

__device__ __forceinline__ Chunk load_chunk(const int64_t *__restrict__ table, int n_tensors,
                                            const int64_t *__restrict__ chunks, int64_t c) {
  Chunk k;
  k.t = static_cast<int>(chunks[c * 3 + 0]);
  k.off = chunks[c * 3 + 1];
  k.n = static_cast<int>(chunks[c * 3 + 2]);
  k.count = table[static_cast<int64_t>(SG_OPTIM_ROW_COUNT) * n_tensors + k.t];
  return k;
}

template <typename T>
__device__ __forceinline__ T *table_ptr(const int64_t *__restrict__ table, int n_tensors, int row, int t) {
  return reinterpret_cast<T *>(static_cast<uintptr_t>(table[static_cast<int64_t>(row) * n_tensors + t]));
}

// Elements [0, head) and [head + 4 * quads, n) of a chunk are scalar, the middle is float4.  The middle exists
// only where every array of the walk has the same address modulo 16 (a parameter that is a view at an odd
// element offset next to freshly allocated states has not: the whole chunk is scalar then).
struct Split {
  int head, quads;
};
__device__ __forceinline__ Split split_chunk(int n, const void *a, const void *b, const void *c, const void *d) {
  const uintptr_t ra = reinterpret_cast<uintptr_t>(a) & 15;
  bool same = true;
  if (b) same = same && (reinterpret_cast<uintptr_t>(b) & 15) == ra;
  if (c) same = same && (reinterpret_cast<uintptr_t>(c) & 15) == ra;
  if (d) same = same && (reinterpret_cast<uintptr_t>(d) & 15) == ra;
  Split s;
  if (!same || (ra & 3) != 0) {
    s.head = n, s.quads = 0;
    return s;
  }
  const int h = static_cast<int>(((16 - ra) & 15) >> 2);
  s.head = h < n ? h : n;
  s.quads = (n - s.head) >> 2;
  return s;
}

__device__ __forceinline__ float inv_scale_of(const float *__restrict__ grad_scale) {
  // GradScaler's own form: scale.double().reciprocal().float()
  return grad_scale ? static_cast<float>(1.0 / static_cast<double>(*grad_scale)) : 1.0f;
}

// b^n for an integer-valued n >= 0, by squaring, in double
__device__ __forceinline__ double pow_int(double b, float n) {
  long long e = n > 0.0f ? static_cast<long long>(n) : 0;
  double r = 1.0;
  while (e) {
    if (e & 1) r *= b;
    b *= b;
    e >>= 1;
  }
  return r;
}

// ---- fixed-order sums (losses.hip's block_sum, two slots) -------------------------------------------------
// CONTRACT: called by every thread of the workgroup from uniform control flow; thread 0 returns with the sums.
__device__ __forceinline__ void block_sum2(double &a, double &b) {
  __shared__ double sh[kOptBlock / kWave][2];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
  }
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane_id() == 0) sh[wave][0] = a, sh[wave][1] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    a = sh[0][0], b = sh[0][1];
    for (int w = 1; w < kOptBlock / kWave; ++w) a += sh[w][0], b += sh[w][1];
  }
}

// ---- gradient norm -----------------------------------------------------------------------------------------
__device__ __forceinline__ void norm_acc(float g, double inv, double &sum, double &bad) {
  const double x = static_cast<double>(g) * inv;      // (exact: 24 x 24 bits)
  sum += x * x;
  // not finite <=> x - x is NaN
  bad += (x - x == 0.0) ? 0.0 : 1.0;
}

__global__ void __launch_bounds__(kOptBlock) grad_norm_kernel(const int64_t *__restrict__ table, int n_tensors,
                                                             const int64_t *__restrict__ chunks, int64_t n_chunks,
                                                             const float *__restrict__ grad_scale,
                                                             double *__restrict__ partial) {
  const double inv = static_cast<double>(inv_scale_of(grad_scale));
  double sum = 0.0, bad = 0.0;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const Chunk k = load_chunk(table, n_tensors, chunks, c);
    const float *g = table_ptr<const float>(table, n_tensors, SG_OPTIM_ROW_GRAD, k.t) + k.off;
    const Split s = split_chunk(k.n, g, nullptr, nullptr, nullptr);
    const float4 *gq = reinterpret_cast<const float4 *>(g + s.head);
    for (int q0 = 0; q0 < s.quads; q0 += kOptFlight * kOptBlock) {
      float4 v[kOptFlight];
#pragma unroll
      for (int j = 0; j < kOptFlight; ++j) {
        const int q = q0 + j * kOptBlock + static_cast<int>(threadIdx.x);
        v[j] = q < s.quads ? gq[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      }
#pragma unroll
      for (int j = 0; j < kOptFlight; ++j) {
        norm_acc(v[j].x, inv, sum, bad);
        norm_acc(v[j].y, inv, sum, bad);
        norm_acc(v[j].z, inv, sum, bad);
        norm_acc(v[j].w, inv, sum, bad);
      }
    }
    const int tail0 = s.head + 4 * s.quads;
    for (int i = threadIdx.x; i < s.head; i += kOptBlock) norm_acc(g[i], inv, sum, bad);
    for (int i = tail0 + threadIdx.x; i < k.n; i += kOptBlock) norm_acc(g[i], inv, sum, bad);
  }
  block_sum2(sum, bad);
  if (threadIdx.x == 0) partial[blockIdx.x * 2 + 0] = sum, partial[blockIdx.x * 2 + 1] = bad;
}

// out: [0] = norm, [1] = clip_coef, [2] = found_inf (0 / 1), [3] = 0
__global__ void __launch_bounds__(kOptBlock) grad_norm_finalize_kernel(const double *__restrict__ partial, int nblocks,
                                                                      float max_norm, float *__restrict__ out) {
  double sum = 0.0, bad = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += kOptBlock) sum += partial[b * 2 + 0], bad += partial[b * 2 + 1];
  block_sum2(sum, bad);
  if (threadIdx.x != 0) return;
  const float norm = static_cast<float>(sqrt(sum));
  // clip_grad_norm_: max_norm / (total_norm + 1e-6) in float32, clamped to 1 (a NaN norm stays NaN)
  const float coef = max_norm / (norm + 1e-6f);
  out[0] = norm;
  out[1] = coef > 1.0f ? 1.0f : coef;
  out[2] = bad != 0.0 ? 1.0f : 0.0f;
  out[3] = 0.0f;
}

// ---- the walk shared by the step kernels -------------------------------------------------------------------
// F::elem(p, g, m, v) updates one element in registers; the walk loads, stores and zeroes.
template <bool kHasM, bool kHasV, typename F>
__device__ __forceinline__ void walk_chunk(const F &f, int n, float *__restrict__ p, float *__restrict__ g,
                                           float *__restrict__ m, float *__restrict__ v, bool zero_grad) {
  const Split s = split_chunk(n, p, g, kHasM ? m : nullptr, kHasV ? v : nullptr);
  float4 *pq = reinterpret_cast<float4 *>(p + s.head), *gq = reinterpret_cast<float4 *>(g + s.head);
  float4 *mq = kHasM ? reinterpret_cast<float4 *>(m + s.head) : nullptr;
  float4 *vq = kHasV ? reinterpret_cast<float4 *>(v + s.head) : nullptr;
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (int q0 = 0; q0 < s.quads; q0 += kOptFlight * kOptBlock) {
    float4 P[kOptFlight], G[kOptFlight], M[kOptFlight], V[kOptFlight];
#pragma unroll
    for (int j = 0; j < kOptFlight; ++j) {
      const int q = q0 + j * kOptBlock + static_cast<int>(threadIdx.x);
      const bool in = q < s.quads;
      P[j] = in ? pq[q] : zero;
      G[j] = in ? gq[q] : zero;
      M[j] = (kHasM && in) ? mq[q] : zero;
      V[j] = (kHasV && in) ? vq[q] : zero;
    }
#pragma unroll
    for (int j = 0; j < kOptFlight; ++j) {
      const int q = q0 + j * kOptBlock + static_cast<int>(threadIdx.x);
      if (q >= s.quads) continue;
      f.elem(P[j].x, G[j].x, M[j].x, V[j].x);
      f.elem(P[j].y, G[j].y, M[j].y, V[j].y);
      f.elem(P[j].z, G[j].z, M[j].z, V[j].z);
      f.elem(P[j].w, G[j].w, M[j].w, V[j].w);
      pq[q] = P[j];
      if (kHasM) mq[q] = M[j];
      if (kHasV) vq[q] = V[j];
      if (zero_grad) gq[q] = zero;
    }
  }
  const int tail0 = s.head + 4 * s.quads;
  for (int r = 0; r < 2; ++r) {
    const int lo = r == 0 ? 0 : tail0, hi = r == 0 ? s.head : n;
    for (int i = lo + threadIdx.x; i < hi; i += kOptBlock) {
      float pe = p[i], ge = g[i], me = kHasM ? m[i] : 0.0f, ve = kHasV ? v[i] : 0.0f;
      f.elem(pe, ge, me, ve);
      p[i] = pe;
      if (kHasM) m[i] = me;
      if (kHasV) v[i] = ve;
      if (zero_grad) g[i] = 0.0f;
    }
  }
}

// CONTRACT: called by every thread of the workgroup from uniform control flow, after its stores of a chunk.
// old_step is what the chunk read.  Every thread loads the counter itself at the top of the chunk, and the waves
// of a workgroup are not in step with each other between chunks: a wave that is still on its way into this chunk
// must not find the counter advanced by a wave that is already through it (above kOptMaxBlocks chunks a workgroup
// walks several chunks back to back).  So the barrier comes first, for every tensor: behind it the workgroup's
// loads of this chunk, the counter among them, have returned.
// Single-chunk tensors then advance their counter directly.  Otherwise the chunks of a tensor count themselves in
// arrive[t]; the last one advances the counter and zeroes arrive[t] for the next launch.  Every chunk has read
// the counter (its update depends on it) before it counts itself, so none can read the advanced value.
__device__ __forceinline__ void chunk_done(const Chunk &k, float old_step, float *__restrict__ step,
                                           int32_t *__restrict__ arrive) {
  const int64_t n_of_tensor = (k.count + kOptChunk - 1) / kOptChunk;
  __syncthreads();
  if (n_of_tensor <= 1) {
    if (threadIdx.x == 0) *step = old_step + 1.0f;
    return;
  }
  if (threadIdx.x == 0) {
    const int before = atomicAdd(arrive + k.t, 1);
    if (before == static_cast<int>(n_of_tensor) - 1) {
      arrive[k.t] = 0;
      *step = old_step + 1.0f;
    }
  }
}

struct AdamElem {
  double inv, coef, wd, decay, w1, b2, w2, step_size, bc2_sqrt, eps;
  bool adamw;
  __device__ __forceinline__ void elem(float &p, float g, float &m, float &v) const {
    double pd = p, gd = static_cast<double>(g) * inv * coef, md = m, vd = v;
    if (adamw)
      pd *= decay;                      // p *= 1 - lr * wd
    else if (wd != 0.0)
      gd += wd * pd;                    // g += wd * p
    md = md + w1 * (gd - md);           // lerp(m, g, 1 - b1)
    vd = b2 * vd + w2 * gd * gd;
    pd -= step_size * (md / (sqrt(vd) / bc2_sqrt + eps));
    p = static_cast<float>(pd), m = static_cast<float>(md), v = static_cast<float>(vd);
  }
};

__global__ void __launch_bounds__(kOptBlock) adam_step_kernel(const int64_t *__restrict__ table, int n_tensors,
                                                             const int64_t *__restrict__ chunks, int64_t n_chunks,
                                                             double lr, double beta1, double beta2, double eps,
                                                             double weight_decay, int adamw,
                                                             const float *__restrict__ grad_scale,
                                                             const float *__restrict__ found_inf,
                                                             const float *__restrict__ clip_coef, int zero_grad,
                                                             int32_t *__restrict__ arrive) {
  if (found_inf && *found_inf != 0.0f) return;      // a skipped step writes nothing
  AdamElem f;
  f.inv = static_cast<double>(inv_scale_of(grad_scale));
  f.coef = clip_coef ? static_cast<double>(*clip_coef) : 1.0;
  f.wd = weight_decay, f.decay = 1.0 - lr * weight_decay, f.adamw = adamw != 0;
  f.w1 = 1.0 - beta1, f.b2 = beta2, f.w2 = 1.0 - beta2, f.eps = eps;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const Chunk k = load_chunk(table, n_tensors, chunks, c);
    float *step = table_ptr<float>(table, n_tensors, SG_OPTIM_ROW_STEP, k.t);
    const float old_step = *step;
    const float now = old_step + 1.0f;
    f.step_size = lr / (1.0 - pow_int(beta1, now));
    f.bc2_sqrt = sqrt(1.0 - pow_int(beta2, now));
    walk_chunk<true, true>(f, k.n, table_ptr<float>(table, n_tensors, SG_OPTIM_ROW_PARAM, k.t) + k.off,
                           table_ptr<float>(table, n_tensors, SG_OPTIM_ROW_GRAD, k.t) + k.off,
                           table_ptr<float>(table, n_tensors, SG_OPTIM_ROW_STATE0, k.t) + k.off,
                           table_ptr<float>(table, n_tensors, SG_OPTIM_ROW_STATE1, k.t) + k.off, zero_grad != 0);
    chunk_done(k, old_step, step, arrive);
  }
}

struct SgdElem {
  double inv, coef, wd, lr, momentum, damp;      // damp = 1 - dampening
  bool has_momentum, nesterov, first;
  __device__ __forceinline__ void elem(float &p, float g, float &m, float &) const {
    double pd = p, gd = static_cast<double>(g) * inv * coef;
    if (wd != 0.0) gd += wd * pd;
    if (has_momentum) {
      const double bd = first ? gd : momentum * static_cast<double>(m) + damp * gd;
      m = static_cast<float>(bd);
      gd = nesterov ? gd + momentum * bd : bd;
    }
    p = static_cast<float>(pd - lr * gd);
  }
};

template <bool kHasM>
__global__ void __launch_bounds__(kOptBlock) sgd_step_kernel(const int64_t *__restrict__ table, int n_tensors,
                                                            const int64_t *__restrict__ chunks, int64_t n_chunks,
                                                            double lr, double momentum, double dampening,
                                                            double weight_decay, int nesterov,
                                                            const float *__restrict__ grad_scale,
                                                            const float *__restrict__ found_inf,
                                                            const float *__restrict__ clip_coef, int zero_grad,
                                                            int32_t *__restrict__ arrive) {
  if (found_inf && *found_inf != 0.0f) return;
  SgdElem f;
  f.inv = static_cast<double>(inv_scale_of(grad_scale));
  f.coef = clip_coef ? static_cast<double>(*clip_coef) : 1.0;
  f.wd = weight_decay, f.lr = lr, f.momentum = momentum, f.damp = 1.0 - dampening;
  f.has_momentum = kHasM, f.nesterov = nesterov != 0;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const Chunk k = load_chunk(table, n_tensors, chunks, c);
    float *step = table_ptr<float>(table, n_tensors, SG_OPTIM_ROW_STEP, k.t);
    const float old_step = *step;
    f.first = old_step == 0.0f;      // torch: the momentum buffer starts as a copy of the gradient
    walk_chunk<kHasM, false>(f, k.n, table_ptr<float>(table, n_tensors, SG_OPTIM_ROW_PARAM, k.t) + k.off,
                             table_ptr<float>(table, n_tensors, SG_OPTIM_ROW_GRAD, k.t) + k.off,
                             kHasM ? table_ptr<float>(table, n_tensors, SG_OPTIM_ROW_STATE0, k.t) + k.off : nullptr,
                             nullptr, zero_grad != 0);
    chunk_done(k, old_step, step, arrive);
  }
}

__global__ void __launch_bounds__(kOptBlock) scale_grads_kernel(const int64_t *__restrict__ table, int n_tensors,
                                                               const int64_t *__restrict__ chunks, int64_t n_chunks,
                                                               const float *__restrict__ coef_p) {
  const float coef = *coef_p;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const Chunk k = load_chunk(table, n_tensors, chunks, c);
    float *g = table_ptr<float>(table, n_tensors, SG_OPTIM_ROW_GRAD, k.t) + k.off;
    const Split s = split_chunk(k.n, g, nullptr, nullptr, nullptr);
    float4 *gq = reinterpret_cast<float4 *>(g + s.head);
    for (int q0 = 0; q0 < s.quads; q0 += kOptFlight * kOptBlock) {
      float4 v[kOptFlight];
#pragma unroll
      for (int j = 0; j < kOptFlight; ++j) {
        const int q = q0 + j * kOptBlock + static_cast<int>(threadIdx.x);
        v[j] = q < s.quads ? gq[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      }
#pragma unroll
      for (int j = 0; j < kOptFlight; ++j) {
        const int q = q0 + j * kOptBlock + static_cast<int>(threadIdx.x);
        if (q < s.quads) gq[q] = make_float4(v[j].x * coef, v[j].y * coef, v[j].z * coef, v[j].w * coef);
      }
    }
    const int tail0 = s.head + 4 * s.quads;
    for (int i = threadIdx.x; i < s.head; i += kOptBlock) g[i] *= coef;
    for (int i = tail0 + threadIdx.x; i < k.n; i += kOptBlock) g[i] *= coef;
  }
}

static int tables_check(const char *who, const int64_t *table, int n_tensors, const int64_t *chunks,
                        int64_t n_chunks) {
  SG_REQUIRE(n_tensors >= 0 && n_chunks >= 0, "%s: n_tensors = %d, n_chunks = %lld", who, n_tensors,
             static_cast<long long>(n_chunks));
  SG_REQUIRE(n_chunks == 0 || (table && chunks && n_tensors > 0), "%s: null table with %lld chunks of %d tensors", who,
             static_cast<long long>(n_chunks), n_tensors);
  return SG_OK;
}

static bool is_prob(double b) { return b >= 0.0 && b < 1.0; }

}  // namespace sg

// ---- C ABI -------------------------------------------------------------------------------------------------
using namespace sg;

extern "C" int sg_optim_chunk_elems(void) { return kOptChunk; }

extern "C" size_t sg_optim_workspace_bytes(void) { return optim_ws_bytes(); }

extern "C" int64_t sg_optim_plan(const int64_t *counts, int n_tensors, int64_t *chunks, int64_t chunk_capacity) {
  const char *who = "sg_optim_plan";
  SG_REQUIRE(n_tensors >= 0 && chunk_capacity >= 0, "%s: n_tensors = %d, chunk_capacity = %lld", who, n_tensors,
             static_cast<long long>(chunk_capacity));
  SG_REQUIRE(n_tensors == 0 || counts, "%s: null counts with %d tensors", who, n_tensors);
  SG_REQUIRE(chunk_capacity == 0 || chunks, "%s: null chunks with capacity %lld", who,
             static_cast<long long>(chunk_capacity));
  int64_t n = 0;
  for (int t = 0; t < n_tensors; ++t) {
    SG_REQUIRE(counts[t] >= 0, "%s: counts[%d] = %lld", who, t, static_cast<long long>(counts[t]));
    for (int64_t off = 0; off < counts[t]; off += kOptChunk, ++n) {
      if (n >= chunk_capacity) continue;      // (counting only)
      const int64_t left = counts[t] - off;
      chunks[n * 3 + 0] = t;
      chunks[n * 3 + 1] = off;
      chunks[n * 3 + 2] = left < kOptChunk ? left : kOptChunk;
    }
  }
  if (chunk_capacity != 0 && n > chunk_capacity) {
    set_error("%s: %lld chunks do not fit chunk_capacity = %lld", who, static_cast<long long>(n),
              static_cast<long long>(chunk_capacity));
    return SG_ERR_WORKSPACE;
  }
  return n;
}

extern "C" int sg_optim_grad_norm(const int64_t *table, int n_tensors, const int64_t *chunks, int64_t n_chunks,
                                  const float *grad_scale, float max_norm, float *out, void *ws, size_t ws_bytes,
                                  sg_stream_t stream) {
  const char *who = "sg_optim_grad_norm";
  const int rc = tables_check(who, table, n_tensors, chunks, n_chunks);
  if (rc != SG_OK) return rc;
  SG_REQUIRE(max_norm >= 0.0f, "%s: max_norm = %g", who, static_cast<double>(max_norm));
  SG_REQUIRE(out && ws, "%s: null out / ws", who);
  if (ws_bytes < optim_ws_bytes()) {
    set_error("%s: workspace %zu < %zu bytes", who, ws_bytes, optim_ws_bytes());
    return SG_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  double *partial = static_cast<double *>(ws);
  if (n_chunks == 0) return SG_OK;      // (nothing to launch: `out` keeps what the caller put there)
  const int grid = static_cast<int>(n_chunks < kOptNormBlocks ? n_chunks : kOptNormBlocks);
  grad_norm_kernel<<<grid, kOptBlock, 0, st>>>(table, n_tensors, chunks, n_chunks, grad_scale, partial);
  const int lrc = check_launch(who);
  if (lrc != SG_OK) return lrc;
  grad_norm_finalize_kernel<<<1, kOptBlock, 0, st>>>(partial, grid, max_norm, out);
  return check_launch(who);
}

static int step_grid(int64_t n_chunks) { return static_cast<int>(n_chunks < kOptMaxBlocks ? n_chunks : kOptMaxBlocks); }

extern "C" int sg_optim_adam_step(const int64_t *table, int n_tensors, const int64_t *chunks, int64_t n_chunks,
                                  double lr, double beta1, double beta2, double eps, double weight_decay, int adamw,
                                  const float *grad_scale, const float *found_inf, const float *clip_coef,
                                  int zero_grad, int32_t *arrive, sg_stream_t stream) {
  const char *who = "sg_optim_adam_step";
  const int rc = tables_check(who, table, n_tensors, chunks, n_chunks);
  if (rc != SG_OK) return rc;
  SG_REQUIRE(lr >= 0.0 && is_prob(beta1) && is_prob(beta2) && eps >= 0.0 && weight_decay >= 0.0,
             "%s: lr = %g, betas = (%g, %g), eps = %g, weight_decay = %g", who, lr, beta1, beta2, eps, weight_decay);
  SG_REQUIRE(n_chunks == 0 || arrive, "%s: null arrive", who);
  if (n_chunks == 0) return SG_OK;
  adam_step_kernel<<<step_grid(n_chunks), kOptBlock, 0, as_stream(stream)>>>(
      table, n_tensors, chunks, n_chunks, lr, beta1, beta2, eps, weight_decay, adamw, grad_scale, found_inf,
      clip_coef, zero_grad, arrive);
  return check_launch(who);
}

extern "C" int sg_optim_sgd_step(const int64_t *table, int n_tensors, const int64_t *chunks, int64_t n_chunks,
                                 double lr, double momentum, double dampening, double weight_decay, int nesterov,
                                 const float *grad_scale, const float *found_inf, const float *clip_coef,
                                 int zero_grad, int32_t *arrive, sg_stream_t stream) {
  const char *who = "sg_optim_sgd_step";
  const int rc = tables_check(who, table, n_tensors, chunks, n_chunks);
  if (rc != SG_OK) return rc;
  SG_REQUIRE(lr >= 0.0 && momentum >= 0.0 && weight_decay >= 0.0, "%s: lr = %g, momentum = %g, weight_decay = %g",
             who, lr, momentum, weight_decay);
  // torch.optim.SGD's own rule
  SG_REQUIRE(!nesterov || (momentum > 0.0 && dampening == 0.0), "%s: nesterov needs momentum > 0 and dampening = 0",
             who);
  SG_REQUIRE(n_chunks == 0 || arrive, "%s: null arrive", who);
  if (n_chunks == 0) return SG_OK;
  hipStream_t st = as_stream(stream);
  if (momentum != 0.0)
    sgd_step_kernel<true><<<step_grid(n_chunks), kOptBlock, 0, st>>>(table, n_tensors, chunks, n_chunks, lr, momentum,
                                                                   dampening, weight_decay, nesterov, grad_scale,
                                                                   found_inf, clip_coef, zero_grad, arrive);
  else
    sgd_step_kernel<false><<<step_grid(n_chunks), kOptBlock, 0, st>>>(table, n_tensors, chunks, n_chunks, lr, momentum,
                                                                    dampening, weight_decay, nesterov, grad_scale,
                                                                    found_inf, clip_coef, zero_grad, arrive);
  return check_launch(who);
}

extern "C" int sg_optim_scale_grads(const int64_t *table, int n_tensors, const int64_t *chunks, int64_t n_chunks,
                                    const float *coef, sg_stream_t stream) {
  const char *who = "sg_optim_scale_grads";
  const int rc = tables_check(who, table, n_tensors, chunks, n_chunks);
  if (rc != SG_OK) return rc;
  SG_REQUIRE(coef, "%s: null coef", who);
  if (n_chunks == 0) return SG_OK;
  scale_grads_kernel<<<step_grid(n_chunks), kOptBlock, 0, as_stream(stream)>>>(table, n_tensors, chunks, n_chunks,
                                                                             coef);
  return check_launch(who);
}
