// ensemble.hip -- several results over the SAME points combined into one: the per-point vote of the semantic labels
// (sg_label_vote), the links between the instances of different passes over one stacked mask matrix
// (sg_mask_group_links, the kernel and the rule of sg_mask_cross_links: cross_links.h) and the per-point vote of the
// member masks of every object (sg_mask_vote).  The rules are stated in include/softgroup_hip.h; the reference has
// no counterpart.
//
// Everything here is integer arithmetic, apart from the one IEEE double division of the link rule
// (-ffp-contract=off); the only atomics are integer (atomicOr on adjacency bits, atomicAdd on populations, whose
// sum does not depend on the order): two calls on the same input give the same bytes.
//
// Every loop is bounded by an argument (k, n, n_total, n_obj, the word count), never by a value read from memory;
// every index read from memory (obj_off, members, member_pass, member_weight) is range-checked before it addresses
// anything, and an entry outside its range is ignored.  No workgroup waits for another one.
#include "common.h"
#include "cross_links.h"

namespace sg {

constexpr int kEnBlock = 256;
constexpr int kEnMaxPasses = 32;
constexpr int kEnMaxWeight = 32767;
constexpr int kEnPlanes = 15;                         // bit-sliced counters: v <= 32767 = 2^15 - 1
constexpr int kEnMaxInst = 16384;
constexpr int kEnLabelBlocks = 4096;                  // grid caps, each walked by a stride loop
constexpr int kEnLinkBlocks = 16384;
constexpr int kEnMaskBlocks = 4096;

// ---- label vote -------------------------------------------------------------------------------------------------
// One thread per point, the K labels of the point in registers (KM = K rounded up to 4, 8, 16 or 32; the loops are
// unrolled so that no array is indexed by a variable), K coalesced loads along n.  For every counted label the
// weights of the passes that say the same are added up: O(K^2) comparisons, no histogram, no LDS.
template <int KM>
__global__ void __launch_bounds__(kEnBlock) label_vote_kernel(const int64_t *__restrict__ labels, int k, int64_t n,
                                                              const int32_t *__restrict__ weights, int64_t ignore,
                                                              int64_t *__restrict__ out) {
  int wt[KM];
#pragma unroll
  for (int p = 0; p < KM; ++p) wt[p] = p < k ? weights[p] : 0;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kEnBlock) + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kEnBlock) {
    int64_t lab[KM];
    bool ok[KM];
#pragma unroll
    for (int p = 0; p < KM; ++p) {
      lab[p] = p < k ? labels[static_cast<int64_t>(p) * n + i] : -1;
      ok[p] = lab[p] >= 0 && lab[p] != ignore;
    }
    int best_c = 0;
    int64_t best_l = 0;
#pragma unroll
    for (int p = 0; p < KM; ++p) {
      if (p < k) {                                                  // (wave-uniform)
        int c = 0;
#pragma unroll
        for (int q = 0; q < KM; ++q) c += ok[q] && lab[q] == lab[p] ? wt[q] : 0;
        if (ok[p] && (c > best_c || (c == best_c && lab[p] < best_l))) best_c = c, best_l = lab[p];
      }
    }
    out[i] = best_c > 0 ? best_l : lab[0];
  }
}

// ---- mask vote ----------------------------------------------------------------------------------------------------
struct MvArgs {
  const uint32_t *bits;                  // [n_total, words]
  const int32_t *obj_off, *members, *member_weight, *member_pass, *need;
  uint32_t *out_bits;                    // [n_obj, words]
  int32_t *npoint;                       // [n_obj], zeroed before the launch
  int64_t n_bits, words, chunks;         // chunks = ceil(words / kEnBlock)
  int n_total, n_obj;
};

// planes += (weight at the bits of x): a ripple-carry addition of 15 bit planes, the carry out of the top one kept
__device__ __forceinline__ void mv_add(uint32_t (&plane)[kEnPlanes], uint32_t &over, uint32_t x, int weight) {
  uint32_t carry = 0;
#pragma unroll
  for (int b = 0; b < kEnPlanes; ++b) {
    const uint32_t add = (weight >> b) & 1 ? x : 0u;
    const uint32_t s = plane[b] ^ add ^ carry;
    carry = (plane[b] & add) | (plane[b] & carry) | (add & carry);
    plane[b] = s;
  }
  over |= carry;
}

// One workgroup per (object, 256 words of its row), a lane owns one output word = 32 points.  The lane walks the
// object's members in (pass) order, ORs the words of one pass and adds the pass's weight into the bit-sliced
// counters of its 32 points; v >= need is decided plane by plane from the top.  Row reads are coalesced, the member
// list is block-uniform; one integer atomicAdd per wave into npoint.
__global__ void __launch_bounds__(kEnBlock) mask_vote_kernel(MvArgs a) {
  const int tid = threadIdx.x;
  const int tail = static_cast<int>(a.n_bits & 31);
  const int64_t items = static_cast<int64_t>(a.n_obj) * a.chunks;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {        // (block-uniform)
    const int o = static_cast<int>(item / a.chunks);
    const int64_t w = (item - static_cast<int64_t>(o) * a.chunks) * kEnBlock + tid;
    const bool live = w < a.words;
    // the member range, clamped into [0, n_total] and made ascending before it bounds the loop
    int lo = a.obj_off[o], hi = a.obj_off[o + 1];
    lo = lo < 0 ? 0 : (lo > a.n_total ? a.n_total : lo);
    hi = hi < lo ? lo : (hi > a.n_total ? a.n_total : hi);
    const int need = a.need[o];
    uint32_t plane[kEnPlanes];
#pragma unroll
    for (int b = 0; b < kEnPlanes; ++b) plane[b] = 0;
    uint32_t over = 0, cur = 0;
    int cur_pass = -1, cur_weight = 0;
    for (int m = lo; m < hi; ++m) {                                 // (at most n_total trips)
      const int g = a.members[m], pass = a.member_pass[m], weight = a.member_weight[m];
      if (g < 0 || g >= a.n_total || pass < 0 || pass >= kEnMaxPasses || weight < 1 || weight > kEnMaxWeight)
        continue;                                                   // an entry outside its range is ignored
      if (pass != cur_pass) {
        if (cur_pass >= 0) mv_add(plane, over, cur, cur_weight);
        cur = 0, cur_pass = pass, cur_weight = weight;
      }
      if (live) cur |= a.bits[static_cast<int64_t>(g) * a.words + w];
    }
    if (cur_pass >= 0) mv_add(plane, over, cur, cur_weight);
    // v >= need, from the top plane: gt = decided greater, eq = equal so far
    uint32_t gt = 0, eq = ~0u;
#pragma unroll
    for (int b = kEnPlanes - 1; b >= 0; --b) {
      const uint32_t nb = (need >> b) & 1 ? ~0u : 0u;
      gt |= eq & plane[b] & ~nb;
      eq &= ~(plane[b] ^ nb);
    }
    uint32_t res = need >= 1 && need <= kEnMaxWeight ? (gt | eq | over) : 0u;
    if (live && w == a.words - 1 && tail) res &= (1u << tail) - 1u;          // bits at and beyond n_bits are 0
    if (!live) res = 0;
    if (live) a.out_bits[static_cast<int64_t>(o) * a.words + w] = res;
    const int total = wave_sum(__popc(res));                        // (every lane is here: the loop is block-uniform)
    if ((tid & 63) == 0 && total) atomicAdd(&a.npoint[o], total);
  }
}

}  // namespace sg

using namespace sg;

extern "C" {

int sg_label_vote(const int64_t *labels, int k, int64_t n, const int32_t *weights, int64_t ignore_label, int64_t *out,
                  sg_stream_t stream_) {
  if (k < 1 || k > kEnMaxPasses || n < 0 || n >= (1LL << 31)) {
    set_error("sg_label_vote: %d passes over %lld points outside the supported range (1 .. %d, < 2^31)", k,
              static_cast<long long>(n), kEnMaxPasses);
    return SG_ERR_UNSUPPORTED;
  }
  if (n == 0) return SG_OK;
  SG_REQUIRE(labels != nullptr && weights != nullptr && out != nullptr, "sg_label_vote: null array");
  SG_REQUIRE(out + n <= labels || labels + static_cast<int64_t>(k) * n <= out, "sg_label_vote: out overlaps labels");
  const int grid = grid_for(n, kEnBlock, kEnLabelBlocks);
  hipStream_t stream = as_stream(stream_);
  if (k <= 4)
    label_vote_kernel<4><<<grid, kEnBlock, 0, stream>>>(labels, k, n, weights, ignore_label, out);
  else if (k <= 8)
    label_vote_kernel<8><<<grid, kEnBlock, 0, stream>>>(labels, k, n, weights, ignore_label, out);
  else if (k <= 16)
    label_vote_kernel<16><<<grid, kEnBlock, 0, stream>>>(labels, k, n, weights, ignore_label, out);
  else
    label_vote_kernel<32><<<grid, kEnBlock, 0, stream>>>(labels, k, n, weights, ignore_label, out);
  return check_launch("sg_label_vote");
}

int sg_mask_group_links(const uint32_t *bits, int n_total, int64_t n_bits, const int32_t *labels, const int32_t *group,
                        double thr, int measure, int min_shared, uint32_t *adj, sg_stream_t stream_) {
  if (n_total < 0 || n_total > kEnMaxInst || n_bits < 0 || n_bits >= (1LL << 31)) {
    set_error("sg_mask_group_links: %d instances, %lld bits outside the supported range (<= %d, < 2^31)", n_total,
              static_cast<long long>(n_bits), kEnMaxInst);
    return SG_ERR_UNSUPPORTED;
  }
  SG_REQUIRE((measure == SG_NMS_IOU || measure == SG_NMS_MIN) && thr == thr,
             "sg_mask_group_links: bad arguments (measure=%d)", measure);
  if (n_total == 0) return SG_OK;
  SG_REQUIRE((n_bits == 0 || bits != nullptr) && labels != nullptr && group != nullptr && adj != nullptr,
             "sg_mask_group_links: null array");
  ClArgs a;
  a.bits_a = a.bits_b = bits, a.labels_a = a.labels_b = labels, a.group_a = a.group_b = group, a.adj = adj;
  a.inter_out = a.cnt_a_out = a.cnt_b_out = nullptr, a.thr = thr;
  a.n_bits = n_bits, a.words = (n_bits + 31) / 32;
  a.n_a = a.n_b = n_total, a.base_a = a.base_b = 0, a.n_total = n_total, a.nw = (n_total + 31) / 32;
  a.measure = measure, a.min_shared = min_shared, a.symmetric = 1;
  cross_links_launch(a, kEnLinkBlocks, as_stream(stream_));         // ONE launch for all pairs of passes
  return check_launch("sg_mask_group_links");
}

int sg_mask_vote(const uint32_t *bits, int n_total, int64_t n_bits, const int32_t *obj_off, const int32_t *members,
                 const int32_t *member_weight, const int32_t *member_pass, const int32_t *need, int n_obj,
                 uint32_t *out_bits, int32_t *npoint, sg_stream_t stream_) {
  if (n_total < 0 || n_total > kEnMaxInst || n_obj < 0 || n_obj > kEnMaxInst || n_bits < 0 || n_bits >= (1LL << 31)) {
    set_error("sg_mask_vote: %d instances, %d objects, %lld bits outside the supported range (<= %d, <= %d, < 2^31)",
              n_total, n_obj, static_cast<long long>(n_bits), kEnMaxInst, kEnMaxInst);
    return SG_ERR_UNSUPPORTED;
  }
  if (n_obj == 0) return SG_OK;
  SG_REQUIRE(obj_off != nullptr && need != nullptr && npoint != nullptr &&
                 (n_total == 0 || (members != nullptr && member_weight != nullptr && member_pass != nullptr)) &&
                 (n_bits == 0 || (out_bits != nullptr && (n_total == 0 || bits != nullptr))),
             "sg_mask_vote: null array");
  SG_REQUIRE(out_bits == nullptr || bits == nullptr || out_bits != bits, "sg_mask_vote: out_bits is bits");
  hipStream_t stream = as_stream(stream_);
  if (hipMemsetAsync(npoint, 0, sizeof(int32_t) * static_cast<size_t>(n_obj), stream) != hipSuccess)
    return check_launch("sg_mask_vote (memset)");
  if (n_bits == 0) return SG_OK;
  MvArgs a;
  a.bits = bits, a.obj_off = obj_off, a.members = members, a.member_weight = member_weight;
  a.member_pass = member_pass, a.need = need, a.out_bits = out_bits, a.npoint = npoint;
  a.n_bits = n_bits, a.words = (n_bits + 31) / 32, a.chunks = (a.words + kEnBlock - 1) / kEnBlock;
  a.n_total = n_total, a.n_obj = n_obj;
  mask_vote_kernel<<<grid_for(static_cast<int64_t>(n_obj) * a.chunks, 1, kEnMaskBlocks), kEnBlock, 0, stream>>>(a);
  return check_launch("sg_mask_vote");
}

}  // extern "C"
