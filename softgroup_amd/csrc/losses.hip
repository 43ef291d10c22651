// losses.hip -- the loss block of forward_train (reference softgroup/model/softgroup.py:152-255) as fused
// kernels: point-wise losses (cross entropy + offset L1), proposal -> class assignment, the proposal-level
// losses (classification CE, IoU-score MSE) and the mask BCE, each with its backward.
//
// The arrays are small (600 k x 20 floats); what the torch form of this block costs is ~40 launches that each
// stream the same rows again.  Here every array is read once per pass.
//
// Sums: every thread accumulates in double, the lanes of a wave meet in a fixed xor butterfly, the waves of a
// workgroup in wave order in LDS, the workgroups write partials [gridDim.x][4] that ONE workgroup of a second,
// tiny kernel adds in a fixed order.  No atomics on floats, no arrival counters (nothing to zero, nothing to
// wrap), so two runs on the same inputs are bit-identical.  The assignment's "later GT overwrites earlier" is an
// integer atomicMax, which is order independent.
#include "common.h"

namespace sg {

constexpr int kLossBlock = 256;
constexpr int kLossMaxBlocks = 1024;
constexpr int kLossMaxC = 64;
constexpr int kLossSlots = 4;      // doubles per workgroup partial

static size_t loss_reduce_bytes() { return align_up(sizeof(double) * kLossSlots * kLossMaxBlocks); }

// ---- fixed-order sums ------------------------------------------------------------------------------------
// CONTRACT: called by every thread of the workgroup from uniform control flow.  Thread 0 returns with the
// workgroup's sums in v.
__device__ __forceinline__ void block_sum(double (&v)[kLossSlots]) {
  __shared__ double sh[kLossBlock / kWave][kLossSlots];
#pragma unroll
  for (int s = 0; s < kLossSlots; ++s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[s] += __shfl_xor(v[s], o, 64);
  }
  const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  __syncthreads();      // (a previous call's reader is done with sh)
  if (lane_id() == 0) {
#pragma unroll
    for (int s = 0; s < kLossSlots; ++s) sh[wave][s] = v[s];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int s = 0; s < kLossSlots; ++s) {
      double a = sh[0][s];
      for (int w = 1; w < nwaves; ++w) a += sh[w][s];
      v[s] = a;
    }
  }
}

__device__ __forceinline__ void store_partial(double (&v)[kLossSlots], double *__restrict__ partial) {
  block_sum(v);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int s = 0; s < kLossSlots; ++s) partial[blockIdx.x * kLossSlots + s] = v[s];
  }
}

enum { kFinPointwise = 0, kFinProposal = 1, kFinMask = 2 };

// out[0..3] = the four sums as float; out[4], out[5] = the losses derived from them
__global__ void __launch_bounds__(kLossBlock) loss_finalize_kernel(const double *__restrict__ partial, int nblocks,
                                                                  int mode, double rows, float *__restrict__ out) {
  double v[kLossSlots] = {0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nblocks; b += kLossBlock) {
#pragma unroll
    for (int s = 0; s < kLossSlots; ++s) v[s] += partial[b * kLossSlots + s];
  }
  block_sum(v);
  if (threadIdx.x != 0) return;
  const float a = static_cast<float>(v[0]), b = static_cast<float>(v[1]);
  const float c = static_cast<float>(v[2]), d = static_cast<float>(v[3]);
  out[0] = a, out[1] = b, out[2] = c, out[3] = d;
  if (mode == kFinPointwise) {          // sum w nll, sum w, sum |delta|, n_pos
    out[4] = a / b;                     // (NaN when every label is ignored, like F.cross_entropy)
    out[5] = c / fmaxf(d, 1.0f);        // (0 when there is no instance point)
  } else if (mode == kFinProposal) {    // sum ce, sum w (s - gt)^2, num_pos, num_neg
    out[4] = a / static_cast<float>(rows);
    out[5] = b / (c + 1.0f);
  } else {                              // sum bce, sum w
    out[4] = a / (b + 1.0f);
    out[5] = 0.0f;
  }
}

static int loss_finalize(const double *partial, int nblocks, int mode, double rows, float *out, hipStream_t st,
                         const char *who) {
  loss_finalize_kernel<<<1, kLossBlock, 0, st>>>(partial, nblocks, mode, rows, out);
  return check_launch(who);
}

// ---- a. / b. point-wise losses -----------------------------------------------------------------------------
// A workgroup of T threads takes tiles of T rows: the tile's scores go through LDS (coalesced global reads and,
// in the backward, coalesced writes; row pitch c | 1 words, so the lanes' row walks hit distinct banks), then
// thread t owns row t.
struct PointwiseArgs {
  const float *scores;
  const int64_t *sem_labels;
  const float *weight;
  int64_t ignore_label;
  const float *pt_offsets, *pt_offset_labels;
  const int64_t *inst_labels;
  int64_t n;
  int c;
};

__device__ __forceinline__ void load_tile(const float *__restrict__ g, float *tile, int64_t base, int rows, int c,
                                          int pitch) {
  const int elems = rows * c;
  const float *src = g + base * c;
  for (int e = threadIdx.x; e < elems; e += blockDim.x) {
    const int r = e / c;
    tile[r * pitch + (e - r * c)] = src[e];
  }
}

__global__ void pointwise_fwd_kernel(PointwiseArgs a, double *__restrict__ partial) {
  extern __shared__ float tile[];
  const int T = blockDim.x, pitch = a.c | 1;
  const int64_t ntiles = (a.n + T - 1) / T;
  double acc[kLossSlots] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t base = t * T;
    const int rows = a.n - base < T ? static_cast<int>(a.n - base) : T;
    __syncthreads();
    load_tile(a.scores, tile, base, rows, a.c, pitch);
    __syncthreads();
    if (static_cast<int>(threadIdx.x) < rows) {
      const int64_t i = base + threadIdx.x;
      const int64_t lab = a.sem_labels[i];
      if (lab != a.ignore_label && lab >= 0 && lab < a.c) {
        const float *row = tile + threadIdx.x * pitch;
        float m = row[0];
        for (int k = 1; k < a.c; ++k) m = fmaxf(m, row[k]);
        float sum = 0.0f;
        for (int k = 0; k < a.c; ++k) sum += expf(row[k] - m);
        const float nll = (m + logf(sum)) - row[lab];
        const float w = a.weight ? a.weight[lab] : 1.0f;
        acc[0] += static_cast<double>(w * nll);
        acc[1] += static_cast<double>(w);
      }
      if (a.inst_labels[i] != a.ignore_label) {
        const float *po = a.pt_offsets + i * 3, *pl = a.pt_offset_labels + i * 3;
        acc[2] += static_cast<double>(fabsf(po[0] - pl[0]) + fabsf(po[1] - pl[1]) + fabsf(po[2] - pl[2]));
        acc[3] += 1.0;
      }
    }
  }
  store_partial(acc, partial);
}

__global__ void pointwise_bwd_kernel(PointwiseArgs a, const float *__restrict__ sums, const float *__restrict__ g_sem,
                                     const float *__restrict__ g_off, float *__restrict__ d_scores,
                                     float *__restrict__ d_offsets) {
  extern __shared__ float tile[];
  const int T = blockDim.x, pitch = a.c | 1;
  const int64_t ntiles = (a.n + T - 1) / T;
  // d (S / W) / d S = g / W first, then times w_i: the order of torch's autograd (NaN for a row of weight 0
  // when W = 0, +-inf otherwise)
  const float gs = g_sem ? *g_sem / sums[1] : 0.0f;
  const float go = g_off ? *g_off / fmaxf(sums[3], 1.0f) : 0.0f;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t base = t * T;
    const int rows = a.n - base < T ? static_cast<int>(a.n - base) : T;
    if (d_scores) {
      __syncthreads();
      load_tile(a.scores, tile, base, rows, a.c, pitch);
      __syncthreads();
    }
    if (static_cast<int>(threadIdx.x) < rows) {
      const int64_t i = base + threadIdx.x;
      if (d_scores) {
        float *row = tile + threadIdx.x * pitch;
        const int64_t lab = a.sem_labels[i];
        if (g_sem && lab != a.ignore_label && lab >= 0 && lab < a.c) {
          float m = row[0];
          for (int k = 1; k < a.c; ++k) m = fmaxf(m, row[k]);
          float sum = 0.0f;
          for (int k = 0; k < a.c; ++k) sum += expf(row[k] - m);
          const float coef = gs * (a.weight ? a.weight[lab] : 1.0f);
          const float inv = 1.0f / sum;
          for (int k = 0; k < a.c; ++k) row[k] = coef * (expf(row[k] - m) * inv - (k == lab ? 1.0f : 0.0f));
        } else {
          for (int k = 0; k < a.c; ++k) row[k] = 0.0f;
        }
      }
      if (d_offsets) {
        float *d = d_offsets + i * 3;
        if (g_off && a.inst_labels[i] != a.ignore_label) {
          const float *po = a.pt_offsets + i * 3, *pl = a.pt_offset_labels + i * 3;
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const float delta = po[j] - pl[j];
            d[j] = delta > 0.0f ? go : (delta < 0.0f ? -go : (delta == 0.0f ? 0.0f : delta * go));   // (NaN stays NaN)
          }
        } else {
          d[0] = d[1] = d[2] = 0.0f;
        }
      }
    }
    if (d_scores) {
      __syncthreads();
      const int elems = rows * a.c;
      float *dst = d_scores + base * a.c;
      for (int e = threadIdx.x; e < elems; e += T) {
        const int r = e / a.c;
        dst[e] = tile[r * pitch + (e - r * a.c)];
      }
    }
  }
}

static int pointwise_threads(int c) { return c <= 32 ? 256 : 128; }      // tile <= 33 KB of LDS

// ---- c. proposal assignment --------------------------------------------------------------------------------
// (value, index) maximum that keeps the LOWEST index among equal values, across a wave
__device__ __forceinline__ void wave_argmax(float &v, int &idx) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (ov > v || (ov == v && oi < idx)) v = ov, idx = oi;
  }
}

// one wave per proposal: arg-max over the GT columns, background columns at IoU -1
__global__ void __launch_bounds__(kLossBlock) assign_rows_kernel(const float *__restrict__ ious,
                                                                const int64_t *__restrict__ instance_cls,
                                                                int64_t ignore_label, float pos_iou_thr,
                                                                int64_t background_label, int n_prop, int n_gt,
                                                                int32_t *__restrict__ assigned, int32_t *__restrict__ lowq,
                                                                int64_t *__restrict__ labels) {
  const int lane = lane_id();
  for (int p = blockIdx.x * (kLossBlock / kWave) + (threadIdx.x >> 6); p < n_prop;
       p += gridDim.x * (kLossBlock / kWave)) {
    float best = -INFINITY;
    int arg = INT32_MAX;
    for (int g = lane; g < n_gt; g += kWave) {
      const float v = instance_cls[g] != ignore_label ? ious[static_cast<int64_t>(p) * n_gt + g] : -1.0f;
      if (v > best) best = v, arg = g;
    }
    wave_argmax(best, arg);
    if (lane == 0) {
      const int a = (best >= pos_iou_thr && arg < n_gt) ? arg : -1;      // (arg >= n_gt: a row of NaNs)
      if (lowq) {
        assigned[p] = a;
        lowq[p] = -1;
      } else {
        labels[p] = a >= 0 ? instance_cls[a] : background_label;
      }
    }
  }
}

// one wave per GT: its best proposal (lowest index among equals); the highest claiming GT index wins a proposal
__global__ void __launch_bounds__(kLossBlock) assign_cols_kernel(const float *__restrict__ ious,
                                                                const int64_t *__restrict__ instance_cls,
                                                                int64_t ignore_label, float min_pos_thr, int n_prop,
                                                                int n_gt, int32_t *__restrict__ lowq) {
  const int lane = lane_id();
  for (int g = blockIdx.x * (kLossBlock / kWave) + (threadIdx.x >> 6); g < n_gt;
       g += gridDim.x * (kLossBlock / kWave)) {
    const bool fg = instance_cls[g] != ignore_label;
    float best = -INFINITY;
    int arg = INT32_MAX;
    for (int p = lane; p < n_prop; p += kWave) {
      const float v = fg ? ious[static_cast<int64_t>(p) * n_gt + g] : -1.0f;
      if (v > best) best = v, arg = p;
    }
    wave_argmax(best, arg);
    if (lane == 0 && best >= min_pos_thr && arg < n_prop) atomicMax(lowq + arg, g);
  }
}

__global__ void __launch_bounds__(kLossBlock) assign_labels_kernel(const int32_t *__restrict__ assigned,
                                                                  const int32_t *__restrict__ lowq,
                                                                  const int64_t *__restrict__ instance_cls,
                                                                  int64_t background_label, int n_prop,
                                                                  int64_t *__restrict__ labels) {
  for (int p = blockIdx.x * kLossBlock + threadIdx.x; p < n_prop; p += gridDim.x * kLossBlock) {
    const int a = lowq[p] >= 0 ? lowq[p] : assigned[p];
    labels[p] = a >= 0 ? instance_cls[a] : background_label;
  }
}

// ---- d. proposal-level losses ------------------------------------------------------------------------------
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one wave per proposal; lane k holds class k (k1 <= 64)
__global__ void __launch_bounds__(kLossBlock) proposal_fwd_kernel(const float *__restrict__ cls_scores,
                                                                 const float *__restrict__ iou_scores,
                                                                 const int64_t *__restrict__ labels,
                                                                 const float *__restrict__ ious_on_pred,
                                                                 const int64_t *__restrict__ instance_cls,
                                                                 int64_t ignore_label, int n_prop, int n_gt, int k1,
                                                                 float *__restrict__ gt_iou,
                                                                 double *__restrict__ partial) {
  const int lane = lane_id();
  double acc[kLossSlots] = {0.0, 0.0, 0.0, 0.0};
  for (int p = blockIdx.x * (kLossBlock / kWave) + (threadIdx.x >> 6); p < n_prop;
       p += gridDim.x * (kLossBlock / kWave)) {
    const int64_t lab = labels[p];
    const float s = lane < k1 ? cls_scores[static_cast<int64_t>(p) * k1 + lane] : -INFINITY;
    const float m = wave_max_f(s);
    const float sum = wave_sum_f(lane < k1 ? expf(s - m) : 0.0f);
    float gt = -INFINITY;
    for (int g = lane; g < n_gt; g += kWave)
      gt = fmaxf(gt, instance_cls[g] != ignore_label ? ious_on_pred[static_cast<int64_t>(p) * n_gt + g] : -1.0f);
    gt = wave_max_f(gt);
    if (lane == 0) {
      gt_iou[p] = gt;
      if (lab >= 0 && lab < k1) acc[0] += static_cast<double>((m + logf(sum)) - cls_scores[static_cast<int64_t>(p) * k1 + lab]);
      if (lab >= 0 && lab < k1 - 1) {
        const float d = iou_scores[static_cast<int64_t>(p) * k1 + lab] - gt;
        acc[1] += static_cast<double>(d * d);
        acc[2] += 1.0;
      } else if (lab >= k1 - 1) {
        acc[3] += 1.0;
      }
    }
  }
  store_partial(acc, partial);
}

__global__ void __launch_bounds__(kLossBlock) proposal_bwd_kernel(const float *__restrict__ cls_scores,
                                                                 const float *__restrict__ iou_scores,
                                                                 const int64_t *__restrict__ labels,
                                                                 const float *__restrict__ gt_iou,
                                                                 const float *__restrict__ sums,
                                                                 const float *__restrict__ g_cls,
                                                                 const float *__restrict__ g_iou, int n_prop, int k1,
                                                                 float *__restrict__ d_cls, float *__restrict__ d_iou) {
  const int lane = lane_id();
  const float gc = g_cls ? *g_cls / static_cast<float>(n_prop) : 0.0f;
  const float gi = g_iou ? *g_iou / (sums[2] + 1.0f) : 0.0f;
  for (int p = blockIdx.x * (kLossBlock / kWave) + (threadIdx.x >> 6); p < n_prop;
       p += gridDim.x * (kLossBlock / kWave)) {
    const int64_t lab = labels[p];
    const int64_t at = static_cast<int64_t>(p) * k1 + lane;
    if (d_cls) {
      const float s = lane < k1 ? cls_scores[at] : -INFINITY;
      const float m = wave_max_f(s);
      const float e = lane < k1 ? expf(s - m) : 0.0f;
      const float sum = wave_sum_f(e);
      if (lane < k1)
        d_cls[at] = (g_cls && lab >= 0 && lab < k1) ? gc * (e / sum - (lane == lab ? 1.0f : 0.0f)) : 0.0f;
    }
    if (d_iou && lane < k1)
      d_iou[at] = (g_iou && lab >= 0 && lab < k1 - 1 && lane == lab) ? gi * 2.0f * (iou_scores[at] - gt_iou[p]) : 0.0f;
  }
}

// ---- e. mask loss ------------------------------------------------------------------------------------------
// The probability, the two logarithms and the gradient are evaluated in double from the fp32 logit and rounded
// once: the formulas are the ones of F.binary_cross_entropy after a sigmoid (the -100 clamp, the 1e-12 floor of
// its backward, the zero gradient where the sigmoid saturates), at the precision of the float64 reference.
__device__ __forceinline__ bool mask_column(const int32_t *__restrict__ batch_idxs, const int64_t *__restrict__ labels,
                                            int64_t i, int n_prop, int k1, int *col) {
  const int b = batch_idxs[i];
  if (b < 0 || b >= n_prop) return false;
  const int64_t c = labels[b];
  if (c < 0 || c >= k1) return false;
  *col = static_cast<int>(c);
  return true;
}

__global__ void __launch_bounds__(kLossBlock) mask_fwd_kernel(const float *__restrict__ mask_scores,
                                                             const int32_t *__restrict__ batch_idxs,
                                                             const int64_t *__restrict__ labels,
                                                             const float *__restrict__ mask_label, int64_t m,
                                                             int n_prop, int k1, float *__restrict__ mask_sig,
                                                             double *__restrict__ partial) {
  double acc[kLossSlots] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kLossBlock) + threadIdx.x; i < m;
       i += static_cast<int64_t>(gridDim.x) * kLossBlock) {
    int col;
    if (!mask_column(batch_idxs, labels, i, n_prop, k1, &col)) {
      mask_sig[i] = 0.0f;
      continue;
    }
    const double p = 1.0 / (1.0 + exp(-static_cast<double>(mask_scores[i * k1 + col])));
    mask_sig[i] = static_cast<float>(p);
    const float y = mask_label[i];
    if (y != -1.0f) {
      const double yd = y;
      acc[0] -= yd * fmax(log(p), -100.0) + (1.0 - yd) * fmax(log1p(-p), -100.0);
      acc[1] += 1.0;
    }
  }
  store_partial(acc, partial);
}

// one thread per element of d_mask_scores [m, k1]: coalesced stores of whole rows, one non-zero per row
__global__ void __launch_bounds__(kLossBlock) mask_bwd_kernel(const float *__restrict__ mask_scores,
                                                             const int32_t *__restrict__ batch_idxs,
                                                             const int64_t *__restrict__ labels,
                                                             const float *__restrict__ mask_label,
                                                             const float *__restrict__ sums,
                                                             const float *__restrict__ g_mask, int64_t m, int n_prop,
                                                             int k1, float *__restrict__ d_mask_scores) {
  const double g = g_mask ? static_cast<double>(*g_mask / (sums[1] + 1.0f)) : 0.0;
  const int64_t total = m * k1;
  for (int64_t e = blockIdx.x * static_cast<int64_t>(kLossBlock) + threadIdx.x; e < total;
       e += static_cast<int64_t>(gridDim.x) * kLossBlock) {
    const int64_t i = e / k1;
    const int k = static_cast<int>(e - i * k1);
    int col;
    float out = 0.0f;
    if (g_mask && mask_column(batch_idxs, labels, i, n_prop, k1, &col) && col == k) {
      const float y = mask_label[i];
      if (y != -1.0f) {
        const double p = 1.0 / (1.0 + exp(-static_cast<double>(mask_scores[e])));
        const double pq = p * (1.0 - p);
        out = static_cast<float>(g * (p - static_cast<double>(y)) / fmax(pq, 1e-12) * pq);
      }
    }
    d_mask_scores[e] = out;
  }
}

}  // namespace sg

// ---- C ABI -------------------------------------------------------------------------------------------------
using namespace sg;

extern "C" size_t sg_loss_reduce_workspace_bytes(void) { return loss_reduce_bytes(); }

extern "C" size_t sg_assign_proposals_workspace_bytes(int n_proposal) {
  return 2 * align_up(sizeof(int32_t) * static_cast<size_t>(n_proposal > 0 ? n_proposal : 0)) + 256;
}

static int pointwise_check(const char *who, const float *scores, const int64_t *sem_labels, const float *pt_offsets,
                           const float *pt_offset_labels, const int64_t *inst_labels, int64_t n, int c) {
  SG_REQUIRE(n >= 0 && c >= 1, "%s: n = %lld, c = %d", who, static_cast<long long>(n), c);
  if (c > kLossMaxC) {
    set_error("%s: c = %d above %d classes", who, c, kLossMaxC);
    return SG_ERR_UNSUPPORTED;
  }
  SG_REQUIRE(n == 0 || (scores && sem_labels && pt_offsets && pt_offset_labels && inst_labels), "%s: null input", who);
  return SG_OK;
}

extern "C" int sg_pointwise_loss_fwd(const float *semantic_scores, const int64_t *semantic_labels, const float *weight,
                                     int64_t ignore_label, const float *pt_offsets, const float *pt_offset_labels,
                                     const int64_t *instance_labels, int64_t n, int c, float *out, void *ws,
                                     size_t ws_bytes, sg_stream_t stream) {
  const char *who = "sg_pointwise_loss_fwd";
  const int rc = pointwise_check(who, semantic_scores, semantic_labels, pt_offsets, pt_offset_labels,
                                 instance_labels, n, c);
  if (rc != SG_OK) return rc;
  SG_REQUIRE(out && ws, "%s: null out / ws", who);
  if (ws_bytes < loss_reduce_bytes()) {
    set_error("%s: workspace %zu < %zu bytes", who, ws_bytes, loss_reduce_bytes());
    return SG_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  double *partial = static_cast<double *>(ws);
  const int T = pointwise_threads(c);
  const int grid = grid_for(n, T, kLossMaxBlocks);
  PointwiseArgs a{semantic_scores, semantic_labels, weight, ignore_label, pt_offsets, pt_offset_labels,
                  instance_labels, n, c};
  pointwise_fwd_kernel<<<grid, T, sizeof(float) * T * (c | 1), st>>>(a, partial);
  const int lrc = check_launch(who);
  if (lrc != SG_OK) return lrc;
  return loss_finalize(partial, grid, kFinPointwise, static_cast<double>(n), out, st, who);
}

extern "C" int sg_pointwise_loss_bwd(const float *semantic_scores, const int64_t *semantic_labels, const float *weight,
                                     int64_t ignore_label, const float *pt_offsets, const float *pt_offset_labels,
                                     const int64_t *instance_labels, int64_t n, int c, const float *sums,
                                     const float *g_semantic, const float *g_offset, float *d_scores,
                                     float *d_offsets, sg_stream_t stream) {
  const char *who = "sg_pointwise_loss_bwd";
  const int rc = pointwise_check(who, semantic_scores, semantic_labels, pt_offsets, pt_offset_labels,
                                 instance_labels, n, c);
  if (rc != SG_OK) return rc;
  SG_REQUIRE(sums, "%s: null sums", who);
  if (n == 0 || (!d_scores && !d_offsets)) return SG_OK;
  const int T = pointwise_threads(c);
  PointwiseArgs a{semantic_scores, semantic_labels, weight, ignore_label, pt_offsets, pt_offset_labels,
                  instance_labels, n, c};
  pointwise_bwd_kernel<<<grid_for(n, T, 4 * kLossMaxBlocks), T, sizeof(float) * T * (c | 1), as_stream(stream)>>>(
      a, sums, g_semantic, g_offset, d_scores, d_offsets);
  return check_launch(who);
}

extern "C" int sg_assign_proposals(const float *ious_on_cluster, const int64_t *instance_cls, int64_t ignore_label,
                                   float pos_iou_thr, int match_low_quality, float min_pos_thr,
                                   int64_t background_label, int n_proposal, int n_gt, int64_t *labels, void *ws,
                                   size_t ws_bytes, sg_stream_t stream) {
  const char *who = "sg_assign_proposals";
  SG_REQUIRE(n_proposal >= 0 && n_gt >= 1, "%s: n_proposal = %d, n_gt = %d", who, n_proposal, n_gt);
  SG_REQUIRE(instance_cls && (n_proposal == 0 || (ious_on_cluster && labels)), "%s: null input", who);
  if (n_proposal == 0) return SG_OK;
  hipStream_t st = as_stream(stream);
  const int rows_grid = grid_for(n_proposal, kLossBlock / kWave, kLossMaxBlocks);
  if (!match_low_quality) {
    assign_rows_kernel<<<rows_grid, kLossBlock, 0, st>>>(ious_on_cluster, instance_cls, ignore_label, pos_iou_thr,
                                                         background_label, n_proposal, n_gt, nullptr, nullptr, labels);
    return check_launch(who);
  }
  Workspace w(ws, ws ? ws_bytes : 0);
  int32_t *assigned = w.take<int32_t>(n_proposal), *lowq = w.take<int32_t>(n_proposal);
  if (!assigned || !lowq) {
    set_error("%s: workspace %zu < %zu bytes", who, ws_bytes, sg_assign_proposals_workspace_bytes(n_proposal));
    return SG_ERR_WORKSPACE;
  }
  assign_rows_kernel<<<rows_grid, kLossBlock, 0, st>>>(ious_on_cluster, instance_cls, ignore_label, pos_iou_thr,
                                                       background_label, n_proposal, n_gt, assigned, lowq, labels);
  assign_cols_kernel<<<grid_for(n_gt, kLossBlock / kWave, kLossMaxBlocks), kLossBlock, 0, st>>>(
      ious_on_cluster, instance_cls, ignore_label, min_pos_thr, n_proposal, n_gt, lowq);
  assign_labels_kernel<<<grid_for(n_proposal, kLossBlock, kLossMaxBlocks), kLossBlock, 0, st>>>(
      assigned, lowq, instance_cls, background_label, n_proposal, labels);
  return check_launch(who);
}

static int k1_check(const char *who, int k1) {
  SG_REQUIRE(k1 >= 2, "%s: k1 = %d", who, k1);
  if (k1 > kLossMaxC) {
    set_error("%s: k1 = %d above %d classes", who, k1, kLossMaxC);
    return SG_ERR_UNSUPPORTED;
  }
  return SG_OK;
}

extern "C" int sg_proposal_loss_fwd(const float *cls_scores, const float *iou_scores, const int64_t *labels,
                                    const float *ious_on_pred, const int64_t *instance_cls, int64_t ignore_label,
                                    int n_proposal, int n_gt, int k1, float *gt_iou, float *out, void *ws,
                                    size_t ws_bytes, sg_stream_t stream) {
  const char *who = "sg_proposal_loss_fwd";
  const int rc = k1_check(who, k1);
  if (rc != SG_OK) return rc;
  SG_REQUIRE(n_proposal >= 0 && n_gt >= 1, "%s: n_proposal = %d, n_gt = %d", who, n_proposal, n_gt);
  SG_REQUIRE(instance_cls && out && ws, "%s: null instance_cls / out / ws", who);
  SG_REQUIRE(n_proposal == 0 || (cls_scores && iou_scores && labels && ious_on_pred && gt_iou), "%s: null input", who);
  if (ws_bytes < loss_reduce_bytes()) {
    set_error("%s: workspace %zu < %zu bytes", who, ws_bytes, loss_reduce_bytes());
    return SG_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  double *partial = static_cast<double *>(ws);
  const int grid = grid_for(n_proposal, kLossBlock / kWave, kLossMaxBlocks);
  proposal_fwd_kernel<<<grid, kLossBlock, 0, st>>>(cls_scores, iou_scores, labels, ious_on_pred, instance_cls,
                                                   ignore_label, n_proposal, n_gt, k1, gt_iou, partial);
  const int lrc = check_launch(who);
  if (lrc != SG_OK) return lrc;
  return loss_finalize(partial, grid, kFinProposal, static_cast<double>(n_proposal), out, st, who);
}

extern "C" int sg_proposal_loss_bwd(const float *cls_scores, const float *iou_scores, const int64_t *labels,
                                    const float *gt_iou, const float *sums, const float *g_cls, const float *g_iou,
                                    int n_proposal, int k1, float *d_cls_scores, float *d_iou_scores,
                                    sg_stream_t stream) {
  const char *who = "sg_proposal_loss_bwd";
  const int rc = k1_check(who, k1);
  if (rc != SG_OK) return rc;
  SG_REQUIRE(n_proposal >= 0 && sums, "%s: n_proposal = %d, sums = %p", who, n_proposal, static_cast<const void *>(sums));
  SG_REQUIRE(n_proposal == 0 || (cls_scores && iou_scores && labels && gt_iou), "%s: null input", who);
  if (n_proposal == 0 || (!d_cls_scores && !d_iou_scores)) return SG_OK;
  proposal_bwd_kernel<<<grid_for(n_proposal, kLossBlock / kWave, kLossMaxBlocks), kLossBlock, 0, as_stream(stream)>>>(
      cls_scores, iou_scores, labels, gt_iou, sums, g_cls, g_iou, n_proposal, k1, d_cls_scores, d_iou_scores);
  return check_launch(who);
}

extern "C" int sg_mask_loss_fwd(const float *mask_scores, const int32_t *instance_batch_idxs, const int64_t *labels,
                                const float *mask_label, int64_t m, int n_proposal, int k1, float *mask_sig,
                                float *out, void *ws, size_t ws_bytes, sg_stream_t stream) {
  const char *who = "sg_mask_loss_fwd";
  const int rc = k1_check(who, k1);
  if (rc != SG_OK) return rc;
  SG_REQUIRE(m >= 0 && n_proposal >= 0, "%s: m = %lld, n_proposal = %d", who, static_cast<long long>(m), n_proposal);
  SG_REQUIRE(out && ws, "%s: null out / ws", who);
  SG_REQUIRE(m == 0 || (mask_scores && instance_batch_idxs && mask_label && mask_sig && (labels || n_proposal == 0)),
             "%s: null input", who);
  if (ws_bytes < loss_reduce_bytes()) {
    set_error("%s: workspace %zu < %zu bytes", who, ws_bytes, loss_reduce_bytes());
    return SG_ERR_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  double *partial = static_cast<double *>(ws);
  const int grid = grid_for(m, kLossBlock, kLossMaxBlocks);
  mask_fwd_kernel<<<grid, kLossBlock, 0, st>>>(mask_scores, instance_batch_idxs, labels, mask_label, m, n_proposal, k1,
                                               mask_sig, partial);
  const int lrc = check_launch(who);
  if (lrc != SG_OK) return lrc;
  return loss_finalize(partial, grid, kFinMask, static_cast<double>(m), out, st, who);
}

extern "C" int sg_mask_loss_bwd(const float *mask_scores, const int32_t *instance_batch_idxs, const int64_t *labels,
                                const float *mask_label, const float *sums, const float *g_mask, int64_t m,
                                int n_proposal, int k1, float *d_mask_scores, sg_stream_t stream) {
  const char *who = "sg_mask_loss_bwd";
  const int rc = k1_check(who, k1);
  if (rc != SG_OK) return rc;
  SG_REQUIRE(m >= 0 && n_proposal >= 0 && sums, "%s: m = %lld, n_proposal = %d, sums = %p", who,
             static_cast<long long>(m), n_proposal, static_cast<const void *>(sums));
  SG_REQUIRE(m == 0 || (mask_scores && instance_batch_idxs && mask_label && d_mask_scores && (labels || n_proposal == 0)),
             "%s: null input", who);
  if (m == 0) return SG_OK;
  mask_bwd_kernel<<<grid_for(m * k1, kLossBlock, 8 * kLossMaxBlocks), kLossBlock, 0, as_stream(stream)>>>(
      mask_scores, instance_batch_idxs, labels, mask_label, sums, g_mask, m, n_proposal, k1, d_mask_scores);
  return check_launch(who);
}
