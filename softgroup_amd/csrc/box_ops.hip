// box_ops.hip -- yaw-oriented 3D boxes against each other on gfx950: the IoU matrix of two box lists (sg_box_iou),
// eval_det_cls's matching with that IoU (sg_det_match_obb) and greedy box NMS (sg_box_nms).
//
// The reference has no counterpart: its eval_det scores axis-aligned boxes.  The rules are stated in
// include/softgroup_hip.h; softgroup_amd.ops.boxes.obb_iou_pair is the definition and box_iou_numpy its vectorised
// twin, which every entry here equals byte for byte.  Arithmetic is IEEE double, one operation per written operation
// (built with -ffp-contract=off); the device evaluates no transcendental function -- (cos, sin) come in the box rows.
//
// The one operation underneath is the intersection of two rotated rectangles: rectangle a's four corners are taken
// into b's frame and clipped against b's four half-planes (Sutherland-Hodgman).  The polygon has up to eight vertices
// and a vertex count known only at run time, so a per-thread array would go to scratch memory.  It lives in LDS
// instead: two ping-pong buffers laid out [slot][coordinate][lane] -- 2 x 8 x 2 doubles per lane, 64 KiB for the 256
// lanes of a workgroup, consecutive lanes in consecutive banks.  A lane only ever touches its own column, so there is
// no barrier anywhere.  Every loop has a constant bound and every store a slot below 8, whatever the boxes hold.
//
//   check     a lane per box row: an entry that is not finite or a negative extent sets SG_BOX_FLAG_INVALID.
//   pairs     a lane per (i, j), capped grid and a stride loop; the z reject comes before any clipping.
//   match     a lane per detection over the GT boxes of its (class, image) group, like match_kernel in det_eval.hip;
//             claims by integer atomicMin of the rank, flags in a second pass.
//   NMS       ranks by nms_rank_kernel, a lane per pair i < j sets one bit of the decide matrix [n, ceil(n / 32)]
//             indexed by rank (integer atomicOr), then the one-wave nms_greedy_kernel -- both kernels stay in
//             mask_nms.hip and are reached through nms_greedy.h.
#include "common.h"
#include "nms_greedy.h"

namespace {

constexpr int kBoxBlock = 256;
constexpr int kBoxMaxGrid = 4096;          // pair kernels: at most kBoxMaxGrid * kBoxBlock lanes, then the stride loop
constexpr int kBoxMaxNms = 16384;
constexpr int kBoxMaxPairsLog2 = 30;       // sg_box_iou: n_a * n_b <= 2^30
constexpr int kBoxSlots = 8;
constexpr int kBoxPolyDoubles = 2 * kBoxSlots * 2 * kBoxBlock;      // 64 KiB

struct BoxThresholds {
  double t[SG_DET_MAX_THRESHOLDS];
  int n;
};

__device__ __forceinline__ void load_row(const double *__restrict__ rows, int64_t k, double r[8]) {
#pragma unroll
  for (int c = 0; c < 8; ++c) r[c] = rows[8 * k + c];
}

// (buffer, slot, coordinate) of the calling lane's polygon; `col` = the LDS array + threadIdx.x
__device__ __forceinline__ double *poly_at(double *col, int buf, int slot, int coord) {
  return col + ((buf * kBoxSlots + slot) * 2 + coord) * kBoxBlock;
}

// area(a, b): rectangle a clipped in b's frame (rules 1 - 6)
__device__ __forceinline__ double clip_area(const double a[8], const double b[8], double *col) {
  const double hua = 0.5 * a[3], hva = 0.5 * a[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double su = (k == 1 || k == 2) ? 1.0 : -1.0, sv = k >= 2 ? 1.0 : -1.0;
    const double u = su * hua, v = sv * hva;
    const double x = a[0] + (u * a[6] - v * a[7]);
    const double y = a[1] + (u * a[7] + v * a[6]);
    const double dx = x - b[0], dy = y - b[1];
    *poly_at(col, 1, k, 0) = dx * b[6] + dy * b[7];
    *poly_at(col, 1, k, 1) = dy * b[6] - dx * b[7];
  }
  int n = 4;
  const double hub = 0.5 * b[3], hvb = 0.5 * b[4];
#pragma unroll
  for (int plane = 0; plane < 4; ++plane) {
    const int axis = plane >> 1, src = (plane + 1) & 1, dst = plane & 1;
    const double sign = (plane & 1) ? -1.0 : 1.0, h = axis ? hvb : hub;
    int cnt = 0;
    for (int i = 0; i < kBoxSlots; ++i) {
      if (i >= n) break;
      const int nx = i + 1 < n ? i + 1 : 0;
      const double px = *poly_at(col, src, i, 0), py = *poly_at(col, src, i, 1);
      const double qx = *poly_at(col, src, nx, 0), qy = *poly_at(col, src, nx, 1);
      const double dp = h - sign * (axis ? py : px), dq = h - sign * (axis ? qy : qx);
      const bool p_in = dp >= 0.0, q_in = dq >= 0.0;          // (a NaN is outside)
      if (p_in && cnt < kBoxSlots) {
        *poly_at(col, dst, cnt, 0) = px;
        *poly_at(col, dst, cnt, 1) = py;
        ++cnt;
      }
      if (p_in != q_in && cnt < kBoxSlots) {
        const double t = dp / (dp - dq);
        const double rx = px + t * (qx - px), ry = py + t * (qy - py);
        *poly_at(col, dst, cnt, 0) = axis ? rx : sign * h;
        *poly_at(col, dst, cnt, 1) = axis ? sign * h : ry;
        ++cnt;
      }
    }
    n = cnt;
    if (n == 0) return 0.0;
  }
  if (n < 3) return 0.0;
  // (four planes: the polygon is in buffer 1)
  const double x0 = *poly_at(col, 1, 0, 0), y0 = *poly_at(col, 1, 0, 1);
  double acc = 0.0;
  for (int i = 1; i < kBoxSlots - 1; ++i) {
    if (i > n - 2) break;
    const double xi = *poly_at(col, 1, i, 0), yi = *poly_at(col, 1, i, 1);
    const double xj = *poly_at(col, 1, i + 1, 0), yj = *poly_at(col, 1, i + 1, 1);
    acc = acc + ((xi - x0) * (yj - y0) - (xj - x0) * (yi - y0));
  }
  return 0.5 * fabs(acc);
}

__device__ __forceinline__ double box_iou_pair(const double a[8], const double b[8], int mode, double *col) {
  double h = 1.0;
  if (mode == SG_BOX_IOU_3D) {
    const double lo_a = a[2] - 0.5 * a[5], lo_b = b[2] - 0.5 * b[5];
    const double hi_a = a[2] + 0.5 * a[5], hi_b = b[2] + 0.5 * b[5];
    const double zlo = lo_a > lo_b ? lo_a : lo_b, zhi = hi_a < hi_b ? hi_a : hi_b;
    h = zhi - zlo;
    if (!(h > 0.0)) return 0.0;
  }
  const double area = clip_area(a, b, col);
  if (!(area > 0.0)) return 0.0;
  double inter, uni;
  if (mode == SG_BOX_IOU_3D) {
    inter = area * h;
    uni = ((a[3] * a[4]) * a[5] + (b[3] * b[4]) * b[5]) - inter;
  } else {
    inter = area;
    uni = (a[3] * a[4] + b[3] * b[4]) - area;
  }
  if (!(uni > 0.0)) return 0.0;
  return inter / uni;
}

__global__ void __launch_bounds__(kBoxBlock) box_check_kernel(const double *__restrict__ rows, int64_t n,
                                                              int32_t *__restrict__ flags) {
  for (int64_t k = blockIdx.x * static_cast<int64_t>(kBoxBlock) + threadIdx.x; k < n;
       k += static_cast<int64_t>(gridDim.x) * kBoxBlock) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) ok = ok && isfinite(rows[8 * k + c]);
#pragma unroll
    for (int c = 3; c < 6; ++c) ok = ok && rows[8 * k + c] >= 0.0;
    if (!ok) atomicOr(flags, SG_BOX_FLAG_INVALID);
  }
}

// iou[i * n_b + j] = iou(a_i, b_j)
__global__ void __launch_bounds__(kBoxBlock) box_pairs_kernel(const double *__restrict__ a, const double *__restrict__ b,
                                                              int64_t n_b, int64_t n_pairs, int mode,
                                                              double *__restrict__ iou) {
  __shared__ double s_poly[kBoxPolyDoubles];
  double *col = s_poly + threadIdx.x;
  for (int64_t p = blockIdx.x * static_cast<int64_t>(kBoxBlock) + threadIdx.x; p < n_pairs;
       p += static_cast<int64_t>(gridDim.x) * kBoxBlock) {
    const int64_t i = p / n_b, j = p - i * n_b;
    double ra[8], rb[8];
    load_row(a, i, ra);
    load_row(b, j, rb);
    iou[p] = box_iou_pair(ra, rb, mode, col);
  }
}

// (ovmax, jmax) per detection and the claims, as match_kernel of det_eval.hip with the IoU above
__global__ void __launch_bounds__(kBoxBlock) box_match_kernel(const double *__restrict__ det_box,
                                                              const int32_t *__restrict__ det_group,
                                                              const int32_t *__restrict__ det_rank, int64_t n_det,
                                                              const double *__restrict__ gt_box,
                                                              const int64_t *__restrict__ group_off, int64_t n_gt,
                                                              BoxThresholds th, int mode, double *__restrict__ ovmax_out,
                                                              int64_t *__restrict__ jmax_out,
                                                              int32_t *__restrict__ claim) {
  __shared__ double s_poly[kBoxPolyDoubles];
  double *col = s_poly + threadIdx.x;
  for (int64_t d = blockIdx.x * static_cast<int64_t>(kBoxBlock) + threadIdx.x; d < n_det;
       d += static_cast<int64_t>(gridDim.x) * kBoxBlock) {
    double bb[8];
    load_row(det_box, d, bb);
    const int32_t g = det_group[d];
    double ovmax = -INFINITY;
    int64_t jmax = -1;
    int64_t j0 = group_off[g], j1 = group_off[g + 1];
    j0 = j0 < 0 ? 0 : j0;                                      // (a bad offset table reads no row outside gt_box)
    j1 = j1 > n_gt ? n_gt : j1;
    for (int64_t j = j0; j < j1; ++j) {
      double gb[8];
      load_row(gt_box, j, gb);
      const double iou = box_iou_pair(bb, gb, mode, col);
      if (iou > ovmax) {
        ovmax = iou;
        jmax = j;
      }
    }
    ovmax_out[d] = ovmax;
    jmax_out[d] = jmax;
    for (int k = 0; k < th.n; ++k)
      if (ovmax > th.t[k]) atomicMin(claim + k * n_gt + jmax, det_rank[d]);
  }
}

// tp[thr * n_det + d] = 1 when d won its claim
__global__ void __launch_bounds__(kBoxBlock) box_flag_kernel(const int32_t *__restrict__ det_rank, int64_t n_det,
                                                             int64_t n_gt, BoxThresholds th,
                                                             const double *__restrict__ ovmax,
                                                             const int64_t *__restrict__ jmax,
                                                             const int32_t *__restrict__ claim,
                                                             uint8_t *__restrict__ tp) {
  for (int64_t d = blockIdx.x * static_cast<int64_t>(kBoxBlock) + threadIdx.x; d < n_det;
       d += static_cast<int64_t>(gridDim.x) * kBoxBlock) {
    const double o = ovmax[d];
    const int64_t j = jmax[d];
    for (int k = 0; k < th.n; ++k)
      tp[k * n_det + d] = (o > th.t[k] && claim[k * n_gt + j] == det_rank[d]) ? 1 : 0;
  }
}

// pairs i <= j of one list: iou(box_i, box_j) into iou_out (both halves) and, for i < j of one label over the
// threshold, the bit (rank of the earlier, rank of the later) of the decide matrix
__global__ void __launch_bounds__(kBoxBlock) box_decide_kernel(const double *__restrict__ boxes, int n,
                                                               const int32_t *__restrict__ labels,
                                                               const int32_t *__restrict__ rank, double thr, int mode,
                                                               uint32_t *__restrict__ decide, int nw,
                                                               double *__restrict__ iou_out) {
  __shared__ double s_poly[kBoxPolyDoubles];
  double *col = s_poly + threadIdx.x;
  const int64_t n_pairs = static_cast<int64_t>(n) * n;
  for (int64_t p = blockIdx.x * static_cast<int64_t>(kBoxBlock) + threadIdx.x; p < n_pairs;
       p += static_cast<int64_t>(gridDim.x) * kBoxBlock) {
    const int i = static_cast<int>(p / n), j = static_cast<int>(p - static_cast<int64_t>(i) * n);
    if (j < i) continue;
    const bool may = i != j && (labels == nullptr || labels[i] == labels[j]);
    if (iou_out == nullptr && !may) continue;
    double ra[8], rb[8];
    load_row(boxes, i, ra);
    load_row(boxes, j, rb);
    const double iou = box_iou_pair(ra, rb, mode, col);
    if (iou_out != nullptr) {
      iou_out[static_cast<int64_t>(i) * n + j] = iou;
      iou_out[static_cast<int64_t>(j) * n + i] = iou;
    }
    if (may && iou > thr) {
      const uint32_t ri = static_cast<uint32_t>(rank[i]), rj = static_cast<uint32_t>(rank[j]);
      const uint32_t first = ri < rj ? ri : rj, later = ri < rj ? rj : ri;
      if (later < static_cast<uint32_t>(n))                    // (ranks are a permutation for finite scores)
        atomicOr(&decide[static_cast<int64_t>(first) * nw + (later >> 5)], 1u << (later & 31));
    }
  }
}

bool mode_ok(int mode) { return mode == SG_BOX_IOU_3D || mode == SG_BOX_IOU_BEV; }

}  // namespace

using namespace sg;

extern "C" {

int sg_box_iou(const double *a, int64_t n_a, const double *b, int64_t n_b, int mode, double *iou, int32_t *flags,
               sg_stream_t stream_) {
  constexpr int64_t kMax = 1LL << kBoxMaxPairsLog2;
  if (n_a < 0 || n_b < 0 || n_a > kMax || n_b > kMax || (n_a > 0 && n_b > kMax / n_a)) {
    set_error("sg_box_iou: %lld x %lld boxes outside the supported range (n_a, n_b >= 0, n_a * n_b <= 2^%d)",
              static_cast<long long>(n_a), static_cast<long long>(n_b), kBoxMaxPairsLog2);
    return SG_ERR_UNSUPPORTED;
  }
  SG_REQUIRE(mode_ok(mode) && flags != nullptr && (n_a == 0 || a != nullptr) && (n_b == 0 || b != nullptr) &&
                 (n_a * n_b == 0 || iou != nullptr),
             "sg_box_iou: bad arguments (mode %d)", mode);
  hipStream_t stream = as_stream(stream_);
  if (n_a > 0) box_check_kernel<<<grid_for(n_a, kBoxBlock, 1024), kBoxBlock, 0, stream>>>(a, n_a, flags);
  if (n_b > 0) box_check_kernel<<<grid_for(n_b, kBoxBlock, 1024), kBoxBlock, 0, stream>>>(b, n_b, flags);
  const int64_t n_pairs = n_a * n_b;
  if (n_pairs > 0)
    box_pairs_kernel<<<grid_for(n_pairs, kBoxBlock, kBoxMaxGrid), kBoxBlock, 0, stream>>>(a, b, n_b, n_pairs, mode, iou);
  return check_launch("sg_box_iou");
}

size_t sg_det_match_obb_workspace_bytes(int64_t n_gt, int n_thresholds) {
  return align_up(static_cast<size_t>(n_gt < 0 ? 0 : n_gt) * (n_thresholds < 0 ? 0 : n_thresholds) * 4);
}

int sg_det_match_obb(const double *det_box, const int32_t *det_group, const int32_t *det_rank, int64_t n_det,
                     const double *gt_box, const int64_t *group_off, int64_t n_gt, const double *thresholds,
                     int n_thresholds, int mode, double *ovmax, int64_t *jmax, uint8_t *tp, void *ws, size_t ws_bytes,
                     sg_stream_t stream_) {
  SG_REQUIRE(n_det >= 0 && n_det < (1LL << 31) && n_gt >= 0 && n_gt < (1LL << 31) && n_thresholds >= 1 &&
                 n_thresholds <= SG_DET_MAX_THRESHOLDS && thresholds && mode_ok(mode) &&
                 (n_det == 0 || (det_box && det_group && det_rank && group_off && ovmax && jmax && tp)) &&
                 (n_gt == 0 || gt_box),
             "sg_det_match_obb: bad arguments");
  SG_REQUIRE(ws_bytes >= sg_det_match_obb_workspace_bytes(n_gt, n_thresholds) && (n_gt == 0 || ws),
             "sg_det_match_obb: workspace too small");
  if (n_det == 0) return SG_OK;
  hipStream_t stream = as_stream(stream_);
  BoxThresholds th;
  th.n = n_thresholds;
  for (int k = 0; k < n_thresholds; ++k) th.t[k] = thresholds[k];
  int32_t *claim = static_cast<int32_t *>(ws);
  if (n_gt > 0) hipMemsetAsync(claim, 0x7F, static_cast<size_t>(n_gt) * n_thresholds * 4, stream);
  const int g = grid_for(n_det, kBoxBlock, kBoxMaxGrid);
  box_match_kernel<<<g, kBoxBlock, 0, stream>>>(det_box, det_group, det_rank, n_det, gt_box, group_off, n_gt, th, mode,
                                                ovmax, jmax, claim);
  box_flag_kernel<<<g, kBoxBlock, 0, stream>>>(det_rank, n_det, n_gt, th, ovmax, jmax, claim, tp);
  return check_launch("sg_det_match_obb");
}

size_t sg_box_nms_workspace_bytes(int n) {
  if (n < 0 || n > kBoxMaxNms) return 0;
  const size_t k = static_cast<size_t>(n), nw = (k + 31) / 32;
  return 2 * align_up(k * 4 + 4) + align_up(k * nw * 4 + 4) + 256;
}

int sg_box_nms(const double *boxes, int n, const float *scores, const int32_t *labels, double thr, int mode,
               int class_agnostic, uint8_t *keep, int32_t *n_keep, double *iou_out, void *ws, size_t ws_bytes,
               sg_stream_t stream_) {
  if (n < 0 || n > kBoxMaxNms) {
    set_error("sg_box_nms: %d boxes outside the supported range (0 <= n <= %d)", n, kBoxMaxNms);
    return SG_ERR_UNSUPPORTED;
  }
  SG_REQUIRE(mode_ok(mode) && n_keep != nullptr && thr == thr, "sg_box_nms: bad arguments (mode %d)", mode);
  SG_REQUIRE(n == 0 || (boxes != nullptr && scores != nullptr && keep != nullptr), "sg_box_nms: null array");
  SG_REQUIRE(ws != nullptr && ws_bytes >= sg_box_nms_workspace_bytes(n), "sg_box_nms: workspace too small");
  hipStream_t stream = as_stream(stream_);
  const int nw = (n + 31) / 32;
  Workspace w(ws, ws_bytes);
  int32_t *rank = w.take<int32_t>(n + 1), *order = w.take<int32_t>(n + 1);
  uint32_t *decide = w.take<uint32_t>(static_cast<size_t>(n) * nw + 1);
  SG_REQUIRE(decide != nullptr, "sg_box_nms: workspace too small");
  FillList f;
  f.add(decide, static_cast<size_t>(n) * nw * 4, 0);
  f.add(n_keep + 1, 4, 0);                                     // the flag word
  fill_many(f, stream);
  if (n > 0) {
    box_check_kernel<<<grid_for(n, kBoxBlock, 1024), kBoxBlock, 0, stream>>>(boxes, n, n_keep + 1);
    nms_rank_launch(scores, n, rank, order, stream);
    box_decide_kernel<<<grid_for(static_cast<int64_t>(n) * n, kBoxBlock, kBoxMaxGrid), kBoxBlock, 0, stream>>>(
        boxes, n, class_agnostic ? nullptr : labels, rank, thr, mode, decide, nw, iou_out);
  }
  nms_greedy_launch(decide, order, n, nw, keep, n_keep, stream);
  return check_launch("sg_box_nms");
}

}  // extern "C"
