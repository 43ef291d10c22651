/*
 * softgroup_hip.h -- C ABI of libsoftgroup_hip.so (MI355X / gfx950).
 *
 * The drop-in boundary for the SoftGroup hot path: plain pointers and sizes, no
 * torch/ATen types.  Each entry point replaces one symbol the reference binds
 * through pybind (softgroup/ops/src/softgroup_api.cpp:8-28) or one piece of the
 * un-vendored spconv 2.1 library the reference model calls
 * (softgroup/model/softgroup.py:60-62, softgroup/model/blocks.py:31-119).
 * The replaced reference interface is cited at every declaration (paths relative
 * to the reference repository root).
 *
 * Conventions
 *   - all `const T* x` / `T* x` arguments are DEVICE pointers unless the name ends in
 *     `_host` or the function name contains `_host`;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every
 *     kernel is launched on it, nothing synchronises unless documented;
 *   - no function allocates device memory: scratch comes from the caller through
 *     (`ws`, `ws_bytes`) sized by the matching `*_workspace_bytes` query;
 *   - return value: SG_OK (0) or a negative SG_ERR_* code; sg_last_error() gives text;
 *   - functions whose output size is data dependent are split into a sizing pass
 *     that writes small int32 "meta" scalars to device memory (the caller reads them
 *     back) and a fill pass.
 */
#ifndef SOFTGROUP_HIP_H
#define SOFTGROUP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *sg_stream_t;

#define SG_OK 0
#define SG_ERR_ARG (-1)
#define SG_ERR_WORKSPACE (-2)
#define SG_ERR_LAUNCH (-3)
#define SG_ERR_UNSUPPORTED (-4)

#define SG_BALLQUERY_MAX_NEIGHBORS 1000 /* bfs_cluster.cu:24 `int idx_temp[1000]` */
#define SG_OCTREE_NUM_NODES 585         /* octree_ball_query.cu:10 */
#define SG_OCTREE_NUM_LEAVES 512        /* octree_ball_query.cu:11 */
#define SG_LISTS_SORTED 1
#define SG_LISTS_RADIUS 2

int sg_version(void);
const char *sg_last_error(void);
/* name/CU count/clock of the current device, for bench records */
int sg_device_info(char *name_host, int name_cap, int *num_cu_host, int *clock_khz_host);

/* Runtime state the library keeps per (device, caller stream) -- the executors' events and pinned read-back
 * words, the conv launches' arrival-counter and ticket pools (8 MB of device
 * memory) -- is created on a stream's first use and normally lives as long as the process.  A caller
 * that retires a stream (a pool of scan threads being resized) calls this once the stream is idle and
 * before destroying it, on the stream's device.  No counterpart in the reference (spconv keeps its
 * workspaces in the torch allocator). */
int sg_stream_release(sg_stream_t stream);
/* A stream of the library's own (hipStreamCreateWithFlags, non-blocking) for a scan worker, and its end:
 * sg_stream_destroy synchronises it, releases its state (sg_stream_release) and destroys it.  Unlike the streams
 * a framework hands out from a fixed pool (torch.cuda.Stream() reuses 32 raw handles per device), such a handle
 * is never shared with a later owner, so releasing its state cannot pull buffers from under somebody else's
 * kernels.  The Python binding wraps it as torch.cuda.ExternalStream and, because PyTorch's caching allocator
 * aborts when a stream it has seen disappears, PARKS a retired worker's stream (sg_stream_release only) for the
 * next pool instead of destroying it; sg_stream_destroy is for hosts without such an allocator. */
int sg_stream_create(sg_stream_t *stream_out);
int sg_stream_destroy(sg_stream_t stream);
/* The same with a dispatch priority: level > 0 the device's highest, 0 its default, < 0 its lowest
 * (hipStreamCreateWithPriority over hipDeviceGetStreamPriorityRange).  For scan workers whose scans should not
 * all advance in lockstep: the scan on the high-priority stream finishes at its stand-alone latency. */
int sg_stream_create_priority(sg_stream_t *stream_out, int level);

/* ------------------------------------------------------------------------------------------
 * Voxelisation index build.  Replaces `voxelize_idx` (softgroup_api.cpp:12,
 * voxelize/voxelize.cpp:11-165; Python: ops/functions.py:168-197).
 * coords: int64 [n, ncol], ncol = 3 or 4 (column 0 = batch index when 4).
 * Voxel id = first-seen order; rule row = [count, ascending point idx..., 0 pad].
 * mode: 4 mean / 3 sum (same indices); 0,1 keep first point, 2 keeps last (voxelize.cpp:127-149).
 * ---------------------------------------------------------------------------------------- */
/* Host (CPU) variant -- what the reference runs inside DataLoader workers (data/custom.py:239).
 * Pass 1 fills input_map[n], returns M and maxActive; pass 2 fills the two outputs. */
int sg_voxelize_idx_host(const int64_t *coords_host, int n, int ncol, int mode,
                         int32_t *input_map_host, int32_t *num_voxels_host,
                         int32_t *max_active_host);
int sg_voxelize_idx_fill_host(const int64_t *coords_host, int n, int ncol, int mode,
                              const int32_t *input_map_host, int num_voxels, int max_active,
                              int64_t *out_coords_host, int32_t *out_map_host);
/* Device variant (used in-model: softgroup.py:494,703).  meta[0]=M, meta[1]=maxActive.
 * `fill` must get the same ws buffer, untouched since `build`. */
size_t sg_voxelize_idx_workspace_bytes(int n);
int sg_voxelize_idx_build(const int64_t *coords, int n, int ncol, int mode, int32_t *input_map,
                          int32_t *meta, void *ws, size_t ws_bytes, sg_stream_t stream);
int sg_voxelize_idx_fill(const int64_t *coords, int n, int ncol, int mode,
                         const int32_t *input_map, int num_voxels, int max_active,
                         int64_t *out_coords, int32_t *out_map, void *ws, size_t ws_bytes,
                         sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Voxel feature pooling.  Replaces `voxelize_fp` / `voxelize_bp` (softgroup_api.cpp:13-14,
 * voxelize/voxelize.cu:10-62; Python ops/functions.py:200-234).
 * out[row,:] = sum_{i=1..rules[row,0]} m * feats[rules[row,i],:], m = 1/count if average.
 * Bit-exact with the reference: sequential order, separate multiply and add.
 * ---------------------------------------------------------------------------------------- */
int sg_voxelize_fp(const float *feats, const int32_t *rules, int num_voxels, int max_active,
                   int channels, int average, float *out, sg_stream_t stream);
/* d_feats must be pre-zeroed by the caller (functions.py:228) */
int sg_voxelize_bp(const float *d_out, const int32_t *rules, int num_voxels, int max_active,
                   int channels, int average, float *d_feats, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Ball query.  Replaces `ballquery_batch_p` (softgroup_api.cpp:19, bfs_cluster/bfs_cluster.cpp:17-31,
 * bfs_cluster.cu:15-101; Python ops/functions.py:237-275).
 * Per point: ascending list of the (at most 1000 smallest) indices k of the same batch with
 * d2(k) < radius^2 (strict), self included.  Two passes give a deterministic CSR:
 *   count : start_len[i,1] = min(cnt,1000); meta[0] = total (int32, saturates at INT32_MAX)
 *   (caller exclusive-scans start_len[:,1] into start_len[:,0] -- sg_exclusive_scan_startlen)
 *   fill  : idx[start .. start+len) = neighbours.
 * All three calls of one query share ONE workspace: the grid lives there, and the count pass parks
 * the finished (sorted) lists of up to 64 entries there, which the fill pass only copies.
 * The reference's `nActive > n*meanActive` retry protocol (functions.py:258-266) is kept in
 * the Python facade; the kernels never truncate.
 * ---------------------------------------------------------------------------------------- */
size_t sg_ballquery_workspace_bytes(int n);
int sg_ballquery_build_grid(const float *xyz, const int32_t *batch_idxs, int n, float radius,
                            void *ws, size_t ws_bytes, sg_stream_t stream);
int sg_ballquery_count(const float *xyz, const int32_t *batch_idxs, int n, float radius,
                       int32_t *start_len, int32_t *meta, void *ws, size_t ws_bytes,
                       sg_stream_t stream);
int sg_ballquery_fill(const float *xyz, const int32_t *batch_idxs, int n, float radius,
                      const int32_t *start_len, int32_t *idx, void *ws, size_t ws_bytes,
                      sg_stream_t stream);
/* start_len[i,0] = sum_{j<i} start_len[j,1]; meta[0] = total.  ws >= sg_scan_workspace_bytes(n) */
size_t sg_scan_workspace_bytes(int n);
int sg_exclusive_scan_startlen(int32_t *start_len, int n, int32_t *meta, void *ws,
                               size_t ws_bytes, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Octree ball query (SoftGroup++).  Replaces `build_and_export_octree` + `octree_ball_query`
 * (softgroup_api.cpp:16-18, octree_ball_query/octree_ball_query.cpp:8-188, .cu:14-147;
 * Python ops/functions.py:14-44).  Fixed 3 levels / 585 nodes / 512 leaves.
 * Neighbour order = leaf export order, then within-leaf order; capped at the first 1000.
 * ---------------------------------------------------------------------------------------- */
int sg_octree_build_host(const float *points_host, const float *xyzwhl_host, int num_points,
                         int num_levels, float *boxes_host, int32_t *pt_inds_host,
                         int32_t *pt_start_len_host);
/* The same export built on the DEVICE (no .cpu() of the coordinates, no host thread): root box =
 * extent of `points` ((max + min) / 2, max - min), 3 levels, identical boxes / pt_inds / pt_start_len
 * (start, length per leaf) to sg_octree_build_host with that root.  boxes float [585, 6], pt_inds
 * int32 [n], pt_start_len int32 [512, 2].  Nothing synchronises. */
size_t sg_octree_build_workspace_bytes(int n);
int sg_octree_build(const float *points, int n, float *boxes, int32_t *pt_inds, int32_t *pt_start_len,
                    void *ws, size_t ws_bytes, sg_stream_t stream);
/* SoftGroup.pyramid_inverse_map (softgroup/model/softgroup.py:500-507): proposals over a class's level
 * voxels (proposals_idx int32 [num_pairs, 2] = (proposal, voxel), proposals of a class disjoint) ->
 * proposals over its points through l2p_map int32 [n_points] (voxel of every point): out_idx int32
 * [<= n_points, 2] = (proposal, point), proposal-major with points ascending (the row order of the
 * reference's dense nonzero), out_offsets int32 [n_prop + 1], *n_out_dev = rows written. */
size_t sg_pyramid_inverse_map_workspace_bytes(int n_points, int n_voxels, int n_prop);
int sg_pyramid_inverse_map(const int32_t *proposals_idx, int64_t num_pairs, int n_prop,
                           const int32_t *l2p_map, int n_points, int n_voxels, int32_t *out_idx,
                           int32_t *out_offsets, int32_t *n_out_dev, void *ws, size_t ws_bytes,
                           sg_stream_t stream);
int sg_octree_ballquery_count(const float *points, const float *boxes, const int32_t *pt_inds,
                              const int32_t *pt_start_len, int n, float radius,
                              int32_t *start_len, sg_stream_t stream);
int sg_octree_ballquery_fill(const float *points, const float *boxes, const int32_t *pt_inds,
                             const int32_t *pt_start_len, int n, float radius,
                             const int32_t *start_len, int32_t *idx, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * BFS clustering (soft grouping).  Replaces `bfs_cluster` (softgroup_api.cpp:20,
 * bfs_cluster/bfs_cluster.cpp:33-126; Python ops/functions.py:278-308) -- CPU single thread in
 * the reference, wavefront-parallel here.  Output identical to the sequential algorithm:
 * seeds ascending, members in FIFO-BFS order, clusters with (float)size >= thr kept, where
 * thr = threshold if class_numpoint_mean == -1 else threshold * class_numpoint_mean.
 * `seg_thr[n_seg]` generalises the single (class_id) call to many classes per launch: point i
 * belongs to segment seg_of_point[i] (NULL = all segment 0) and thr = seg_thr[segment].
 *   label : min-ancestor labelling (directed reachability), sizes, kept clusters
 *   emit  : cluster_idxs int32 [sumNPoint,2] = (cluster_id, point_idx), cluster_offsets [nCluster+1]
 * ---------------------------------------------------------------------------------------- */
/* (14 n-word arrays, the scan workspace, one 8-byte record per edge and -- for n > 16 384, where a cluster
 * too large for one workgroup's replay can exist -- the frontier staging of the multi-workgroup replay:
 * 24 bytes x (n + 131 072)) */
size_t sg_bfs_workspace_bytes(int n, int64_t n_edges);
/* list_flags: SG_LISTS_SORTED  every list is strictly ascending (sg_ballquery_* output);
 *             SG_LISTS_RADIUS  lists come from a radius query, i.e. u in list(v) <=> v in list(u)
 *                              unless one of the two lists is capped at 1000 entries
 *                              (sg_ballquery_* and sg_octree_ballquery_* output).
 *             0 = arbitrary directed lists (every edge is checked for its reverse).
 * SYNCHRONISES `stream`: the number of kept clusters sizes the outputs, so it is returned to
 * host memory (*n_cluster_host, *sum_npoint_host). */
int sg_bfs_cluster_label(const int32_t *bq_idxs, const int32_t *start_len, int n,
                         int64_t n_edges, int list_flags, const int32_t *seg_of_point,
                         const float *seg_thr, int n_seg, int32_t *n_cluster_host,
                         int32_t *sum_npoint_host, void *ws, size_t ws_bytes, sg_stream_t stream);
/* same ws buffer, untouched since sg_bfs_cluster_label */
int sg_bfs_cluster_emit(const int32_t *bq_idxs, const int32_t *start_len, int n, int64_t n_edges,
                        const int32_t *seg_of_point, const float *seg_thr, int n_cluster,
                        int sum_npoint, int32_t *cluster_idxs, int32_t *cluster_offsets, void *ws,
                        size_t ws_bytes, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Segment reductions.  Replace `sec_mean` / `sec_min` / `sec_max` (softgroup_api.cpp:25-27,
 * sec_mean/sec_mean.cu:13-93; Python ops/functions.py:351-438) and `global_avg_pool_fp/bp`
 * (softgroup_api.cpp:22-23, roipool/roipool.cu:12-71; Python ops/functions.py:311-348).
 * inp float32 [S, C], offsets int32 [nP+1] -> out float32 [nP, C].
 * ---------------------------------------------------------------------------------------- */
int sg_sec_mean(const float *inp, const int32_t *offsets, int n_seg, int channels, float *out,
                sg_stream_t stream);
int sg_sec_min(const float *inp, const int32_t *offsets, int n_seg, int channels, float *out,
               sg_stream_t stream);
int sg_sec_max(const float *inp, const int32_t *offsets, int n_seg, int channels, float *out,
               sg_stream_t stream);
int sg_global_avg_pool_fp(const float *feats, const int32_t *offsets, int n_seg, int channels,
                          float *out, sg_stream_t stream);
/* d_feats[i,:] += d_out[p,:] / n_p  (d_feats pre-zeroed by the caller, functions.py:341) */
int sg_global_avg_pool_bp(float *d_feats, const int32_t *offsets, const float *d_out, int n_seg,
                          int channels, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Proposal/GT mask IoU and mask targets (training).  Replace `get_mask_iou_on_cluster`,
 * `get_mask_iou_on_pred`, `get_mask_label` (softgroup_api.cpp:8-10,
 * cal_iou_and_masklabel/cal_iou_and_masklabel.cu:9-164; Python ops/functions.py:47-165).
 * O(S) per-proposal label histogram in LDS instead of the reference's O(nP*nI*|P|);
 * the IoU quotient is evaluated in double and rounded to float like the reference.
 * ---------------------------------------------------------------------------------------- */
int sg_get_mask_iou_on_cluster(const int32_t *proposals_idx, const int32_t *proposals_offset,
                               const int64_t *instance_labels, const int32_t *instance_pointnum,
                               int n_instance, int n_proposal, float *proposals_iou,
                               sg_stream_t stream);
int sg_get_mask_iou_on_pred(const int32_t *proposals_idx, const int32_t *proposals_offset,
                            const int64_t *instance_labels, const int32_t *instance_pointnum,
                            const float *mask_scores_sigmoid, int n_instance, int n_proposal,
                            float *proposals_iou, sg_stream_t stream);
/* mask_label pre-filled with -1 by the caller (functions.py:147) */
int sg_get_mask_label(const int32_t *proposals_idx, const int32_t *proposals_offset,
                      const int64_t *instance_labels, const int64_t *instance_cls,
                      const float *proposals_iou, int n_instance, int n_proposal, float iou_thr,
                      float *mask_label, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Sparse convolution (the spconv.pytorch subset of SURVEY.md 2.4).
 * indices int32 [M,4] = (batch, d0, d1, d2); spatial_shape int32[3] on the host.
 *
 * Rulebooks ("gather tables", output-stationary): nbr[j*K + k] = input row feeding output row
 * j through kernel offset k, or -1.
 *   SubM k3 p1 (SubMConv3d, softgroup.py:61-62, blocks.py:57-70): K=27, k=(dx+1)*9+(dy+1)*3+(dz+1)
 *   strided k2 s2 (SparseConv3d, blocks.py:101-107): output coords = c//2 in first-seen order,
 *       inputs with c//2 >= shape//2 dropped; K=8, k=(c0&1)*4+(c1&1)*2+(c2&1)
 *   inverse k2 (SparseInverseConv3d, blocks.py:114-119): K=8, one entry per row
 *       (k = parity of the fine coordinate, value = parent row) -- built from the saved pair.
 * ---------------------------------------------------------------------------------------- */
size_t sg_spconv_hash_workspace_bytes(int num_rows);
/* builds the coordinate hash in ws, then fills nbr[M,27] */
int sg_spconv_subm_rulebook(const int32_t *indices, int num_rows, const int32_t *spatial_shape_host,
                            int32_t *nbr, void *ws, size_t ws_bytes, sg_stream_t stream);
/* pass 1: in2out[M] (-1 = dropped), meta[0] = M_out.  pass 2: out_indices[M_out,4], child[M_out,8] */
int sg_spconv_down_build(const int32_t *indices, int num_rows, const int32_t *spatial_shape_host,
                         int32_t *in2out, int32_t *meta, void *ws, size_t ws_bytes,
                         sg_stream_t stream);
int sg_spconv_down_fill(const int32_t *indices, int num_rows, const int32_t *in2out,
                        int num_out_rows, int32_t *out_indices, int32_t *child, void *ws,
                        size_t ws_bytes, sg_stream_t stream);
/* inv_nbr[M,8] from (fine indices, in2out) */
int sg_spconv_inverse_rulebook(const int32_t *indices_fine, const int32_t *in2out, int num_rows,
                               int32_t *inv_nbr, sg_stream_t stream);

/* Tile plan for the implicit-GEMM kernel: rows are processed in mask-sorted order so that a
 * 32-row MFMA tile only visits kernel offsets some row of the tile really has.
 * T = ceil(M_out/32) tiles, emitted heaviest first (descending number of offsets) so that the
 * dispatcher spreads heavy and light tiles over the chip (longest-processing-time-first):
 *   order[T*32]       : row ids of every tile, -1 padding.  Rows are sorted by their neighbour mask
 *                       with the bits permuted by offset frequency in this layer (rarest offset =
 *                       most significant bit; ties: lower offset is the more common one)
 *   tile_mask[T + SG_PLAN_HIST_WORDS] : [0, T) OR of the masks of the tile's rows; behind them the
 *                       histogram hist[j] = number of tiles with j offsets (j = 0..32, rest 0): with the
 *                       tiles in descending order it gives a consumer the length of the heavy prefix
 *                       and the position of any (tile, offset) of the list without a search
 *   nbr_tiles[T*32*K] : the tile's gather-table rows copied contiguously (-1 for padding rows)
 * Row order behind the API is untouched: a tile computes rows order[32t .. 32t+31] and stores
 * them back at their own row index.  kvol <= 27.
 * (Developer A/B knob SG_PLAN_ORDER=1|2, read once: rows mask-sorted inside super-blocks of consecutive
 * rows and the tiles dealt to the 8 XCDs in contiguous ranges -- the spatially local plans measured and
 * rejected in round 5; the default 0 is the order described above.) */
#define SG_PLAN_HIST_WORDS 40
size_t sg_spconv_plan_workspace_bytes(int num_out_rows);
int sg_spconv_plan(const int32_t *nbr, int num_out_rows, int kvol, int32_t *order,
                   uint32_t *tile_mask, int32_t *nbr_tiles, void *ws, size_t ws_bytes,
                   sg_stream_t stream);

/* Whole-pyramid index build: all gather tables and tile plans of an n_levels-deep U-Net
 * (level l+1 = SparseConv3d k2 s2 of level l) in a handful of launches and ONE host read-back,
 * instead of one rulebook / plan call chain and one read-back per level (spconv sizes every strided
 * conv's output by its own device->host copy; softgroup/model/blocks.py:131-143 is the UBlock
 * recursion this serves).  Results per level are identical to the per-level entry points above
 * (same first-seen numbering of the coarse sites, same tables, same tile plans).
 *   1. sg_spconv_pyramid_rows : rows_dev[l] = number of sites of level l (rows_dev[0] = num_rows);
 *      the caller reads them back (its only synchronisation) and allocates the per-level outputs;
 *   2. sg_spconv_pyramid_build: fills every pointer of levels[0..n_levels) -- `ws` is the SAME
 *      workspace as in step 1 (it carries the hash tables), `ws2` is scratch of
 *      sg_spconv_pyramid_build_workspace_bytes(levels, n_levels).
 * levels[l]: rows (in); indices [rows,4]; nbr [rows,27] + plan `subm`; and for l < n_levels-1:
 * in2out [rows]; child [rows_{l+1},8] + plan `down` (strided conv l -> l+1); inv [rows,8] + plan
 * `up` (inverse conv l+1 -> l).  A plan of a table with R rows: order [T*32], tile_mask
 * [T + SG_PLAN_HIST_WORDS], nbr_tiles [T*32*K], T = ceil(R/32) (see sg_spconv_plan). */
#define SG_PYRAMID_MAX_LEVELS 10
typedef struct sg_plan_ptrs {
  int32_t *order;
  uint32_t *tile_mask;
  int32_t *nbr_tiles;
} sg_plan_ptrs;
typedef struct sg_pyramid_level {
  int rows;
  int32_t *indices;
  int32_t *nbr;
  sg_plan_ptrs subm;
  int32_t *in2out;
  int32_t *child;
  sg_plan_ptrs down;
  int32_t *inv;
  sg_plan_ptrs up;
} sg_pyramid_level;
size_t sg_spconv_pyramid_workspace_bytes(int num_rows, int n_levels);
int sg_spconv_pyramid_rows(const int32_t *indices, int num_rows, const int32_t *spatial_shape_host,
                           int n_levels, int32_t *rows_dev, void *ws, size_t ws_bytes,
                           sg_stream_t stream);
size_t sg_spconv_pyramid_build_workspace_bytes(const sg_pyramid_level *levels_host, int n_levels);
int sg_spconv_pyramid_build(const int32_t *indices, int num_rows, const int32_t *spatial_shape_host,
                            int n_levels, const sg_pyramid_level *levels_host, void *ws,
                            size_t ws_bytes, void *ws2, size_t ws2_bytes, sg_stream_t stream);

/* Weight packing for the conv kernel: src [Cout, K, Cin] (spconv "OKKKI", the checkpoint layout,
 * tools/convert_checkpoint.py:17-19; src_is_kio = 0) or [K, Cin, Cout] (src_is_kio = 1) ->
 * "k8" [K][ceil(Cin/8)][Cout][8] fp32, zero padded (the 8 reduction steps one lane feeds to 8
 * consecutive MFMAs are one 32-B read), FOLLOWED IN THE SAME BUFFER by the same elements as three
 * bf16 planes h, m, l (w = h + m + l, round to nearest even; 2 bytes per element each) for the
 * split-precision kernel.  The buffer is 2.5x the fp32 block: it MUST be sized with
 * sg_spconv_packed_weight_elems(kvol, cin, cout) (in floats) and filled by sg_spconv_pack_weight --
 * sg_spconv_gather_conv_f32 builds its weight descriptor over that full size and, on the default
 * split path, reads the planes.  Non-finite weights: h carries the Inf/NaN, m and l are NaN-free
 * only for finite values (x - Inf = NaN); a diverged model shows NaN where the fp32-MFMA kernel
 * (sg_spconv_set_arithmetic(0)) would show Inf.
 * src_is_kio = 2 / 3 pack the weights of the TRANSPOSED convolution (the input gradient of a layer)
 * straight from that layer's "OKKKI" tensor, read as src [cin][K][cout] (this call's cin = the
 * layer's Cout and vice versa); 3 also mirrors the kernel offsets (k -> K-1-k: SubMConv3d). */
size_t sg_spconv_packed_weight_elems(int kvol, int cin, int cout);
int sg_spconv_pack_weight(const float *w, int cout, int kvol, int cin, int src_is_kio, float *w_k8,
                          sg_stream_t stream);

/* out[j,:] = post( (residual ? residual[j,:] : 0) + sum_k W[k] . in[nbr[j,k],:] )
 *   post(x) = relu(x * post_scale + post_shift) when post_scale != NULL, identity otherwise: the
 *   eval-mode BatchNorm1d + ReLU that FOLLOWS this conv and precedes the next one in
 *   blocks.py:57-70 (conv_branch: BN, ReLU, conv, BN, ReLU, conv), fused into the epilogue.  `in`
 *   is taken as is (already activated by the producer's epilogue or by sg_bn_relu_f32).
 *   Optional second output out_act = relu(out * act_scale + act_shift): the BatchNorm1d + ReLU of
 *   the NEXT block, when `out` itself is still needed raw (residual identity, skip concat).
 * fp32 in / fp32 accumulate on v_mfma_f32_32x32x2_f32 (exact fp32).  cout % 4 == 0 takes the MFMA
 * path; other shapes the scalar path of the same operator.  order/tile_mask/nbr_tiles from
 * sg_spconv_plan (all NULL = natural order, all offsets, slower general kernel).  cin % 16 == 0 with
 * a plan runs the persistent-workgroup kernel.  Layers too small to fill the chip split the kernel
 * offsets over several units and reduce partial sums from `ws` in a fixed order; pass
 * ws >= sg_spconv_conv_workspace_bytes(num_out_rows, cout) (ws = NULL disables the split). */
size_t sg_spconv_conv_workspace_bytes(int num_out_rows, int cout);
int sg_spconv_gather_conv_f32(const float *in, int num_in_rows, const int32_t *nbr,
                              int num_out_rows, int kvol, int cin, int cout, const float *w_k8,
                              const float *post_scale, const float *post_shift,
                              const float *residual, const float *act_scale,
                              const float *act_shift, float *out_act, const int32_t *order,
                              const uint32_t *tile_mask, const int32_t *nbr_tiles, float *out,
                              void *ws, size_t ws_bytes, sg_stream_t stream);

/* Which launch sg_spconv_gather_conv_f32 would make for a layer of these sizes on the current device,
 * under the process-wide settings in force (sg_spconv_set_combine, the developer knobs of the
 * environment): the library's own launch decision -- the launch path consumes the same record -- read
 * out without launching anything.  Meant for tests, which assert through it that a case reaches the
 * kernel form it is named for.  have_plan: order, tile_mask and nbr_tiles are given (16-byte aligned);
 * ws_bytes: as passed to the conv call (0 = no workspace); arithmetic: 0, 1 or 2 as for
 * sg_spconv_set_arithmetic, -1 = the setting in force.  Reports the stand-alone launch, not the
 * recording of a layer inside an open conv chain.
 *   family: 0 scalar kernel (cout % 4 != 0), 1 general tile kernel, 2 persistent kernel on the fp32
 *     MFMA, 3 persistent kernel, split-precision products, 4 persistent kernel, bf16 operands
 *   blocks_per_unit, vec: tile kernel -- 32-column blocks per wave (1..4), vectorised gather (cin % 16 == 0)
 *   variant, nbw, wv, ck, at: families 3 and 4 -- index into the variant table (-1 otherwise), column
 *     blocks per unit, waves per unit, channels per item, line-wise (1) or fragment-shaped (0) gather
 *   ksplit, k_per_split, combine: slices of the kernel-offset range (1 = none), offsets per slice,
 *     partial sums added inside the launch (1) or by the reduce kernel (0; also 0 when ksplit == 1)
 *   units, col_units, grid, block: work units of the launch, units along cout, workgroups, threads each
 *   num_cu, occupancy: what the grid of a persistent launch was sized with (0 otherwise) */
typedef struct sg_conv_launch_info {
  int family;
  int blocks_per_unit, vec;
  int variant, nbw, wv, ck, at;
  int ksplit, k_per_split, combine;
  int col_units, grid, block;
  int num_cu, occupancy;
  int64_t units;
} sg_conv_launch_info;
int sg_spconv_conv_launch_info(int num_out_rows, int num_in_rows, int kvol, int cin, int cout, int have_plan,
                               size_t ws_bytes, int arithmetic, sg_conv_launch_info *info);

/* Arithmetic of the fp32 sparse convolution's products (process-wide, not thread-safe; meant for
 * tests and A/B measurements): 1 = on the bf16 matrix pipe at fp32 accuracy (operands split three
 * ways, six v_mfma_f32_32x32x16_bf16 per 16-channel slice, fp32 accumulation; dropped terms
 * <= 2^-24 |a b|) -- the default; 0 = v_mfma_f32_32x32x2_f32; 2 = bf16 OPERANDS (activations and
 * weights rounded to nearest-even bf16, one v_mfma_f32_32x32x16_bf16 per slice, fp32 accumulation,
 * fp32 in and out: the precision of gather_conv_bf16 without rounding the stored activations; every
 * layer the persistent kernel takes, the fragment-shaped gather of cin % 32 != 0 included --
 * tests/test_conv_ref_gpu.py holds each variant to the float64 result on rounded operands);
 * -1 = back to the environment (SG_CONV_SPLIT).  No counterpart in the reference: spconv 2.1 multiplies in fp32 (or fp16 under
 * autocast).  Edge behaviour of mode 1: an activation that is Inf, NaN or above the bf16 maximum
 * (3.39e38) yields NaN in every output it touches (x - bf16(x) is Inf - Inf), where fp32 products
 * would give Inf; finite inputs below that are unaffected. */
int sg_spconv_set_arithmetic(int mode);

/* Where the partial sums of a layer whose kernel offsets are split over several workgroups (layers
 * with few output rows) are added up (process-wide, not thread-safe; tests and A/B measurements):
 * 1 = inside the launch, by the last workgroup to arrive at each (tile, column unit), partial tiles
 * added in the fixed order 0 .. ksplit-1 -- the default; 0 = by a second kernel (conv_reduce_kernel),
 * same order, identical results; -1 = back to the environment (SG_CONV_COMBINE). */
int sg_spconv_set_combine(int mode);

/* Lanes per node in the grouping head's list kernels (ball-query count and fill passes, the union-find,
 * edge-record and propagation kernels of the clustering): 64 = one wave per node, the form for lists of
 * 36-140 entries; 8 / 16 / 32 = that many lanes per node and 64 / lanes nodes per wave in lock-step, for
 * scenes whose lists hold a handful of entries.  0 = automatic (chosen per call from the mean list
 * length n_edges / n); a forced value below 32 means 32 for the count pass.  Results are bit-identical
 * for every value.  Process-wide atomic; the initial value is the environment's SG_GROUP_LANES.
 * Returns the previous value, or -1 (SG_ERR text set) for any other argument. */
int sg_grouping_set_lanes(int lanes);

/* Multi-layer conv launches ("conv chain", csrc/spconv_conv.hip): inside sg_unet_forward the layers of
 * the U-Net levels with at most SG_CONV_CHAIN_ROWS rows (default 6144) -- softgroup/model/blocks.py:82-143
 * from the strided conv into such a level down to the deepest level and back up, and a whole U-Net that
 * is that small (the tiny U-Net, softgroup/model/softgroup.py:93-95) -- run as ONE persistent launch per
 * <= 22 layers, with a grid barrier between two layers, instead of one launch per layer.  mode 1 = on,
 * 0 = every layer its own launch (same decomposition, bit-identical results; the default: measured
 * neutral for one scan at a time and slower with several scans in flight, profiles/r06_conv_chain.txt),
 * -1 = back to the environment (SG_CONV_CHAIN).  Process-wide, not thread-safe: tests and A/B measurements.
 * sg_spconv_chain_stats: chain launches and the steps (layers, concats) they carried since process start. */
int sg_spconv_set_chain(int mode);
int sg_spconv_chain_stats(int64_t *launches, int64_t *steps);

/* Measurement hook (bench.py roofline): while enabled, every sg_spconv_gather_conv_f32 call -- from
 * Python or from inside sg_unet_forward -- is bracketed by a HIP event pair on its launch stream.
 * sg_spconv_profile_read waits for the events and returns the summed kernel time and the number of
 * calls since the last sg_spconv_profile(1). */
int sg_spconv_profile(int enable);
int sg_spconv_profile_read(double *total_ms, int *launches);
/* Per call since the last sg_spconv_profile(1), in call order: ms[i] and dims[5*i .. 5*i+4] = num_out_rows,
 * kvol, cin, cout, num_in_rows; at most `cap` entries are written, *calls = number recorded (the profiler is
 * a single-threaded developer hook: one stream at a time). */
int sg_spconv_profile_detail(float *ms, int32_t *dims, int cap, int *calls);

/* ---- point-wise heads (csrc/heads.hip) -------------------------------------------------------
 * Replaces, in SoftGroup.forward_backbone / forward_test (softgroup/model/softgroup.py:374-376,320), the
 * devoxelize gather `output.features[input_map.long()]`, the two MLP heads `semantic_linear` /
 * `offset_linear` (softgroup/model/blocks.py:9-27: Linear, BatchNorm1d, ReLU, Linear) in eval mode and
 * `semantic_scores.max(1)[1]` by one kernel.  sg_mlp2: w1 [C][C] and w2 [out][C] in nn.Linear's [out, in]
 * layout, b1 [C], b2 [out], the eval-mode BatchNorm1d folded to y = x * bn_scale + bn_shift.
 * v2p_map [n_points] int32 or int64 (NULL: identity), channels 16 or 32, semantic->out <= 32,
 * offset->out <= 4.  output_feats [n_points, channels] and semantic_preds [n_points] (int64, first
 * maximum) may be NULL.  fp32 FMA chains in ascending channel order (deterministic). */
typedef struct sg_mlp2 {
  const float *w1, *b1, *bn_scale, *bn_shift, *w2, *b2;
  int out;
} sg_mlp2;
int sg_pointwise_heads(const float *voxel_feats, const void *v2p_map, int v2p_is_int64, int n_points,
                       int channels, const sg_mlp2 *semantic, const sg_mlp2 *offset, float *output_feats,
                       float *semantic_scores, float *pt_offsets, int64_t *semantic_preds,
                       sg_stream_t stream);

/* ---- training side of the sparse convolution (csrc/spconv_train.hip; spconv's autograd reached from
 * tools/train.py:47-58 under autocast) ---------------------------------------------------------
 * bf16 operands, fp32 accumulation (v_mfma_f32_32x32x16_bf16), bf16 result rounded to nearest even:
 *   out[j,:] = bf16( sum_k in[nbr[j,k],:] . W[k] )
 * Weights are packed from the fp32 master copy by sg_spconv_pack_weight_bf16 (layout
 * [K][ceil16(Cin)/8][Cout][8] bf16, zero padded); order / tile_mask / nbr_tiles are the plan of
 * sg_spconv_plan (all three, or none of them and `nbr` [M_out][K] instead).  ws: deep levels split the
 * offsets and need sg_spconv_conv_bf16_workspace_bytes (may be NULL: no split).  The input gradient
 * is the same entry point on the transposed gather table with transposed weights. */
size_t sg_spconv_packed_weight_elems_bf16(int kvol, int cin, int cout);
int sg_spconv_pack_weight_bf16(const float *w, int cout, int kvol, int cin, int src_is_kio,
                               uint16_t *w_k8_bf16, sg_stream_t stream);
size_t sg_spconv_conv_bf16_workspace_bytes(int num_out_rows, int cout);
int sg_spconv_gather_conv_bf16(const uint16_t *in, int num_in_rows, const int32_t *nbr, int num_out_rows,
                               int kvol, int cin, int cout, const uint16_t *w_k8_bf16,
                               const int32_t *order, const uint32_t *tile_mask, const int32_t *nbr_tiles,
                               uint16_t *out, void *ws, size_t ws_bytes, sg_stream_t stream);

/* Which launch sg_spconv_gather_conv_bf16 would make for a layer of these sizes: the entry point's own
 * decision (it consumes the same record), a pure function of its arguments -- nothing is launched and no
 * device is touched.  ws_bytes: as passed to the conv call (0 = no workspace; a workspace too small for
 * the split forces ksplit = 1).  Meant for tests, which assert through it the form a case reaches.
 *   col_units, blocks_per_unit: units along cout, 32-column blocks per unit (1..4: the kernel instantiation)
 *   vec: 16-byte gathers (cin % 16 == 0) or element loads
 *   ksplit, k_per_split: slices of the kernel-offset range (1 = none), offsets per slice
 *   num_tiles, units, grid, block: 32-row tiles, waves of work, workgroups, threads each
 *   ws_used: bytes of the workspace the launch writes (0 when ksplit == 1) */
typedef struct sg_conv_bf16_launch_info {
  int col_units, blocks_per_unit, vec;
  int ksplit, k_per_split;
  int num_tiles, grid, block;
  int64_t units;
  int64_t ws_used;
} sg_conv_bf16_launch_info;
int sg_spconv_conv_bf16_launch_info(int num_out_rows, int kvol, int cin, int cout, size_t ws_bytes,
                                    sg_conv_bf16_launch_info *info);

/* Weight gradient: dw_kio[k][ci][co] = sum_j in[nbr[j,k]][ci] * g_out[j][co]  ([K][Cin][Cout] fp32,
 * overwritten).  in / g_out are fp32, or bf16 when the matching flag is set (widened on load; products
 * and sums are fp32).  Row chunks are accumulated separately and added in chunk order: the result is
 * bit-identical from run to run.  ws: sg_spconv_wgrad_workspace_bytes. */
/* nbr_t is the gather table transposed to [K][M_out] (sg_spconv_transpose_table; one per rulebook,
 * shared by all convs that use it): the kernel reads one offset's column at a time. */
int sg_spconv_transpose_table(const int32_t *nbr, int num_out_rows, int kvol, int32_t *nbr_t,
                              sg_stream_t stream);
size_t sg_spconv_wgrad_workspace_bytes(int num_out_rows, int kvol, int cin, int cout);
int sg_spconv_wgrad(const void *in, int in_is_bf16, const void *g_out, int g_is_bf16, const int32_t *nbr_t,
                    int num_out_rows, int kvol, int cin, int cout, float *dw_kio, void *ws,
                    size_t ws_bytes, sg_stream_t stream);

/* The decomposition sg_spconv_wgrad (and its workspace query) would use for such a layer; a pure function
 * of the shape, nothing is launched and no device is touched.
 *   vi, vo: input / gradient channels per lane (1 | 2: the kernel instantiation)
 *   nst, zs: 32 vi x 32 vo supertiles of the (cin, cout) range, workgroups along z that share them
 *   rows, chunks: rows per chunk, chunks
 *   csplit: pieces the centre offset's chunks are cut into (1 = none)
 *   rs: row split inside a workgroup (4 | 2: the waves' accumulators meet in LDS; 1: whole supertiles per wave) */
typedef struct sg_wgrad_launch_info {
  int vi, vo, nst, zs;
  int rows, chunks, csplit, rs;
} sg_wgrad_launch_info;
int sg_spconv_wgrad_launch_info(int num_out_rows, int kvol, int cin, int cout, sg_wgrad_launch_info *info);

/* ------------------------------------------------------------------------------------------
 * Native executor of the sparse U-Net (inference): the whole of
 *   [input_conv] -> UBlock -> [output BatchNorm1d + ReLU]
 * (softgroup/model/softgroup.py:60-65 backbone, :93-95 tiny U-Net; modules of
 * softgroup/model/blocks.py:44-143) in one call: rulebooks, plans and convolutions are launched
 * back to back from C++, device memory comes from the caller's arena.  All pointers are device
 * pointers; weights are packed with sg_spconv_pack_weight, BatchNorm1d is passed in eval form
 * y = x*scale + shift.
 * ---------------------------------------------------------------------------------------- */
typedef struct sg_unet_block {     /* ResidualBlock, blocks.py:44-79 */
  int cin, cout;
  const float *bn1_scale, *bn1_shift;   /* [cin]  conv_branch.0 */
  const float *w1;                      /* SubMConv3d(cin, cout)   conv_branch.2 */
  const float *bn2_scale, *bn2_shift;   /* [cout] conv_branch.3 */
  const float *w2;                      /* SubMConv3d(cout, cout)  conv_branch.5 */
  const float *w_i;                     /* i_branch 1x1 conv (cin != cout) or NULL */
} sg_unet_block;
typedef struct sg_unet_level {     /* UBlock, blocks.py:82-143 */
  int planes, n_blocks;
  const sg_unet_block *blocks;                                /* [n_blocks] */
  const sg_unet_block *tail;                                  /* [n_blocks] blocks_tail, NULL on the deepest level */
  const float *down_bn_scale, *down_bn_shift, *down_w;        /* conv:   BN, ReLU, SparseConv3d(planes, next, k2 s2) */
  const float *up_bn_scale, *up_bn_shift, *up_w;              /* deconv: BN, ReLU, SparseInverseConv3d(next, planes, k2) */
} sg_unet_level;
typedef struct sg_unet_desc {
  int n_levels;
  const sg_unet_level *levels;       /* host array, outermost first */
  int input_cin;
  const float *input_w;              /* SubMConv3d(input_cin, planes[0]) before the UBlock, or NULL */
  const float *out_bn_scale, *out_bn_shift;   /* BatchNorm1d + ReLU after the UBlock, or NULL */
  int input_cin_packed;              /* Cin `input_w` was packed for: 0 or input_cin = as is; a larger
                                        multiple of 16 (weights zero-padded along Cin before packing)
                                        makes the executor convolve a zero-padded copy of the features
                                        on the persistent MFMA kernel instead of the general one */
  int arithmetic;                    /* 0 = the process-wide conv arithmetic (fp32 products); 2 = bf16
                                        operands for this call's convolutions (sg_spconv_set_arithmetic's
                                        mode 2, scoped to the call and the calling thread), activations
                                        fp32 in memory; 3 = bf16 operands AND bf16 activations between the
                                        layers (needs input_w and planes % 32 == 0 on every level, else
                                        it runs as 2): what spconv does with a frozen backbone under the
                                        reference's autocast (tools/train.py:47).  `feats` and `out` stay fp32 */
} sg_unet_desc;
/* upper bound of the arena sg_unet_forward needs for num_rows input voxels */
size_t sg_unet_arena_bytes(const sg_unet_desc *desc, int num_rows);
/* feats [num_rows, input_cin or planes[0]], indices int32 [num_rows,4], out [num_rows, planes[0]].
 * One host synchronisation per call (the row counts of all levels, read back from an internal
 * stream right at the start). */
int sg_unet_forward(const sg_unet_desc *desc, const float *feats, const int32_t *indices,
                    int num_rows, const int32_t *spatial_shape_host, float *out, void *arena,
                    size_t arena_bytes, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Native TRAINING executor of the same U-Net (the DDP training step, tools/train.py:44-62 ->
 * SoftGroup.forward_train, softgroup.py:113-150: tiny U-Net of the refinement head always, the
 * backbone when it is not in `fixed_modules`).  The reference trains these modules through spconv's
 * autograd functions and torch.nn.BatchNorm1d in train() mode, one interpreter round trip and
 * several launches per layer; here
 *   sg_unet_train_forward   runs the whole forward -- BatchNorm1d with BATCH statistics (biased
 *                           variance for the normalisation, running_mean / running_var updated with
 *                           `momentum`, unbiased variance, as torch does), ReLU, the convolutions --
 *                           and records what the backward needs (activations, statistics, tables) in
 *                           the caller's arena and in a host-side tape;
 *   sg_unet_train_backward  consumes the tape: input gradients by the forward kernel on the
 *                           transposed rulebooks, weight gradients by sg_spconv_wgrad, BatchNorm1d
 *                           gradients from fp64 column sums.  Deterministic: no floating-point atomics.
 * Weights and their gradients are the module's own tensors in the checkpoint layout [Cout][K][Cin]
 * (packing happens inside); a NULL gradient pointer skips that gradient (frozen parameter).
 * ---------------------------------------------------------------------------------------- */
typedef struct sg_train_bn {          /* BatchNorm1d(c) in train() mode; weight == NULL: absent */
  const float *weight, *bias;         /* [c] */
  float *running_mean, *running_var;  /* [c], updated in place by the forward */
  float momentum, eps;
  float *g_weight, *g_bias;           /* [c] written by the backward, or NULL */
} sg_train_bn;
typedef struct sg_train_conv {        /* bias-free sparse conv; w == NULL: absent */
  const float *w;                     /* [Cout][K][Cin] */
  float *g_w;                         /* same layout, written by the backward, or NULL */
} sg_train_conv;
typedef struct sg_unet_train_block {  /* ResidualBlock, blocks.py:44-79 */
  int cin, cout;
  sg_train_bn bn1, bn2;
  sg_train_conv c1, c2, ci;           /* ci: 1x1 conv of the identity branch (cin != cout) */
} sg_unet_train_block;
typedef struct sg_unet_train_level {  /* UBlock, blocks.py:82-143 */
  int planes, n_blocks;
  const sg_unet_train_block *blocks, *tail;      /* [n_blocks]; tail NULL on the deepest level */
  sg_train_bn down_bn, up_bn;
  sg_train_conv down, up;
} sg_unet_train_level;
typedef struct sg_unet_train_desc {
  int n_levels;
  const sg_unet_train_level *levels;  /* host array, outermost first */
  int input_cin;
  sg_train_conv input;                /* SubMConv3d(input_cin, planes[0]) before the UBlock, or absent */
  sg_train_bn out_bn;                 /* BatchNorm1d + ReLU after the UBlock, or absent */
  int arithmetic;                     /* as sg_unet_desc.arithmetic (0 | 2), forward and input gradients */
} sg_unet_train_desc;
/* Arena: index tables + every activation of the forward + the gradients of the backward, bump
 * allocated and alive until the backward has run.  *arena_needed (if not NULL) receives the exact
 * size for this input once the level row counts are known; SG_ERR_WORKSPACE = call again with at
 * least that much.  sg_unet_train_arena_hint: a first guess from the row count alone. */
size_t sg_unet_train_arena_hint(const sg_unet_train_desc *desc, int num_rows);
int sg_unet_train_forward(const sg_unet_train_desc *desc, const float *feats, const int32_t *indices,
                          int num_rows, const int32_t *spatial_shape_host, float *out, void *arena,
                          size_t arena_bytes, size_t *arena_needed, void **tape, sg_stream_t stream);
/* g_out [num_rows, planes[0]]; g_feats [num_rows, input_cin or planes[0]] or NULL.  Parameter
 * gradients go to the pointers of the descriptor the forward was given (they must still be valid).
 * Frees the tape, whatever it returns. */
int sg_unet_train_backward(void *tape, const float *g_out, float *g_feats, sg_stream_t stream);
/* a forward whose backward will never run */
void sg_unet_train_release(void *tape);

/* Fused eval-mode BatchNorm1d + ReLU over [M, C] rows (output_layer, softgroup.py:65):
 * out = relu(x*scale + shift) (relu optional). */
int sg_bn_relu_f32(const float *x, const float *scale, const float *shift, int64_t num_rows,
                   int channels, int relu, float *out, sg_stream_t stream);

/* Row gather: out[i,:] = in[index[i],:]  (devoxelize, softgroup.py:374; feats[c_idxs], :677) */
int sg_gather_rows_f32(const float *in, const int32_t *index, int64_t num_out_rows, int channels,
                       float *out, sg_stream_t stream);
int sg_gather_rows_i64idx_f32(const float *in, const int64_t *index, int64_t num_out_rows,
                              int channels, float *out, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Instance extraction for the inference result (SoftGroup.get_instances, softgroup.py:537-604),
 * all instance classes at once, without the reference's dense int32 [nProposal, N] mask per class.
 *   proposals_idx int32 [S,2] = (proposal, point), mask_scores f32 [S, stride] (stride >= n_classes)
 *   sg_instance_npoint: npoint[p*n_classes + i] = #{pairs of proposal p with mask_scores[e,i] >
 *       mask_thr}  (softgroup.py:569-570,584: the row sums of the dense mask)
 *   sg_instance_runs: inst_of[i*n_prop + p] = output index of the kept (class i, proposal p)
 *       instance or -1 (the caller applies cls_score_thr / min_npoint, softgroup.py:573-588, and
 *       numbers the survivors in the reference's order: class-major, proposal-ascending).
 *       Produces the runs of consecutive points of every kept instance's mask in ascending point
 *       order: runs of instance k = [bounds[k], bounds[k+1]) of starts[] / ends[] (0-based,
 *       end exclusive) -- the input of sg_rle_format_host (lens = ends - starts).  Runs past
 *       runs_capacity are dropped (bounds still count them: check bounds[n_kept] <= capacity;
 *       sum of the kept instances' npoint is always enough).
 * ---------------------------------------------------------------------------------------- */
int sg_instance_npoint(const int32_t *proposals_idx, const float *mask_scores, int64_t num_pairs,
                       int stride, int n_classes, float mask_thr, int n_prop, int32_t *npoint,
                       sg_stream_t stream);
size_t sg_instance_runs_workspace_bytes(int n_kept, int n_points);
int sg_instance_runs(const int32_t *proposals_idx, const float *mask_scores, int64_t num_pairs,
                     int stride, int n_classes, float mask_thr, const int32_t *inst_of, int n_prop,
                     int n_kept, int n_points, int32_t *starts, int32_t *ends, int64_t *bounds,
                     int64_t runs_capacity, void *ws, size_t ws_bytes, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Instance-mask run-length strings in the reference's wire format (softgroup/util/rle.py:5-19,
 * called per instance from softgroup.py:595-603): "start len start len ..." with 1-based starts.
 * runs of instance g = [bounds[g], bounds[g+1]) of (starts, lens), all host int64.
 * Text of instance g = out[out_offsets[g] .. out_offsets[g+1]) (no terminators);
 * out_capacity >= sg_rle_format_bound(total_runs, digits of the largest number).
 * ---------------------------------------------------------------------------------------- */
int64_t sg_rle_format_bound(int64_t total_runs, int digits);
int sg_rle_format_host(const int64_t *starts_host, const int64_t *lens_host,
                       const int64_t *bounds_host, int n_groups, char *out_host,
                       int64_t out_capacity, int64_t *out_offsets_host);
/* The same text produced on the device from the output of sg_instance_runs, without a host round trip
 * in between (the run count is read from bounds[n_inst] on the device; run_capacity = the capacity
 * given to sg_instance_runs, length = mask length): text (uint8, >= sg_rle_format_device_text_bytes)
 * holds "start len " for every run in order; instance g's string is
 * text[text_off[g] .. text_off[g+1] - 1) (the space after its last run excluded; empty when it has
 * no run).  Only text[0 .. text_off[n_inst]) and the n_inst+1 offsets have to travel to the host. */
size_t sg_rle_format_device_workspace_bytes(int64_t run_capacity);
int64_t sg_rle_format_device_text_bytes(int64_t run_capacity, int64_t length);
int sg_rle_format_device(const int32_t *starts, const int32_t *ends, const int64_t *bounds, int n_inst,
                         int64_t run_capacity, int64_t length, uint8_t *text, int64_t text_capacity,
                         int64_t *text_off, void *ws, size_t ws_bytes, sg_stream_t stream);
/* same text from the output of sg_instance_runs (int32 starts and exclusive ends, copied to the host) */
int sg_rle_format_runs_host(const int32_t *starts_host, const int32_t *ends_host,
                            const int64_t *bounds_host, int n_groups, char *out_host,
                            int64_t out_capacity, int64_t *out_offsets_host);

/* ------------------------------------------------------------------------------------------
 * Panoptic fusion (SoftGroup.panoptic_fusion, softgroup/model/softgroup.py:606-639) over the bit rows
 * of the kept instances (row k = N-bit mask of instance k, ceil(N/32) words per row; the rows
 * sg_instance_runs builds, see sg_instances_result.bits): instances are visited in `order`
 * (descending confidence -- the caller sorts, like the reference's np.argsort(scores)[::-1]); one
 * whose overlap with already pasted points exceeds skip_iou (intersect / (npoint + 1e-5) > skip_iou,
 * evaluated in double) is skipped, otherwise its free points take the next panoptic id (from 1) and
 * class label_id[k] + cls_offset.  out[i] = (class & 0xFFFF) | (id << 16); points of thing classes
 * (class >= thing_class_min; the reference hard-codes 11) without an id become semantic_classes.
 * semantic_preds int64 [N].  ws >= sg_panoptic_fusion_workspace_bytes. */
size_t sg_panoptic_fusion_workspace_bytes(int n_inst, int n_points);
int sg_panoptic_fusion(const uint32_t *bits, int n_inst, int n_points, const int32_t *order,
                       const int32_t *label_id, const int64_t *semantic_preds, int cls_offset,
                       double skip_iou, int semantic_classes, int thing_class_min, uint32_t *out,
                       void *ws, size_t ws_bytes, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Greedy mask non-maximum suppression over bit rows (csrc/mask_nms.hip).  The reference has NO counterpart:
 * its get_instances returns one instance per (proposal, class) pair and nothing de-duplicates them.  This
 * stage is new and opt-in (test_cfg.nms); nothing calls it unless asked.
 *
 * bits: uint32 [n_inst, ceil(n_points / 32)], point i of mask k = bit i % 32 of word i / 32 of row k (the rows
 * of sg_instances_result.bits); bits at and beyond n_points are ignored.  scores float32 [n_inst], all finite;
 * labels int32 [n_inst], NULL = class-agnostic (as class_agnostic != 0).
 *
 * ORDER: descending score, and among equal scores (-0.0 equals 0.0) the LOWER index first.  This is not the
 * rule of the panoptic fusion and of the pictures, which read an ascending argsort backwards (`[::-1]`: the
 * higher index first).
 * LOOP: the masks are visited in that order; a mask not yet suppressed is kept and suppresses every later mask
 * j of the order that is not yet suppressed, has the same label (unless class-agnostic) and has
 * inter / den > thr, strictly: one IEEE double division of the two integers, den = cnt_i + cnt_j - inter for
 * SG_NMS_IOU and min(cnt_i, cnt_j) for SG_NMS_MIN.  den == 0 suppresses nothing (an empty mask is always
 * kept), and a suppressed mask suppresses nobody.
 * keep uint8 [n_inst] (1 = kept) in the original index order, *n_keep (device int32) = their number.
 * inter_out (may be NULL): int32 [n_inst, n_inst] intersections in original indices, populations on the diagonal.
 *
 * RANGE: n_inst <= 16384 and n_points < 2^31; beyond it the call returns SG_ERR_UNSUPPORTED and
 * sg_mask_nms_workspace_bytes returns 0 -- nothing is truncated.  Nothing synchronises, there is no host
 * read-back and no float atomic: two calls on the same inputs give the same bytes. */
#define SG_NMS_IOU 0
#define SG_NMS_MIN 1
size_t sg_mask_nms_workspace_bytes(int n_inst, int64_t n_points);
int sg_mask_nms(const uint32_t *bits, int n_inst, int64_t n_points, const float *scores, const int32_t *labels,
                double thr, int measure, int class_agnostic, uint8_t *keep, int32_t *n_keep, int32_t *inter_out,
                void *ws, size_t ws_bytes, sg_stream_t stream);
/* Bit rows (the layout above, every word of every row written) from runs: int32 starts and exclusive ends,
 * ascending and disjoint inside a mask, runs of mask k = [bounds[k], bounds[k+1]) of the n_runs runs -- what
 * sg_instance_runs and sg_mask_text_runs take, and sg_inst_rle_parse's slots with ends = start + len.  The
 * expansion sg_viz_paint_runs does (csrc/viz_io.hip). */
int sg_mask_bits_from_runs(const int32_t *starts, const int32_t *ends, const int64_t *bounds, int64_t n_runs,
                           int n_inst, int64_t n_points, uint32_t *bits, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Masks cut into their spatially connected components (csrc/mask_split.hip).  The reference has NO counterpart:
 * nothing in its get_instances looks at geometry, so a mask may be an object plus stray points elsewhere, or two
 * objects of one class welded into one proposal.  This stage is new and opt-in (test_cfg.split); nothing calls it
 * unless asked.  softgroup_amd.ops.split.mask_components_numpy is the definition, the kernels equal it.
 *
 * INPUTS: xyz float32 [n_points, 3] (device); bits uint32 [n_inst, ceil(n_points / 32)], the rows of sg_mask_nms
 * (point i = bit i % 32 of word i / 32, bits at and beyond n_points ignored); radius a finite double > 0 whose
 * square is finite; min_npoint >= 1; mode SG_SPLIT_ALL ('split') or SG_SPLIT_LARGEST ('largest').
 * ADJACENCY: inside ONE mask, points p != q are adjacent when, with dx = (double)x_p - (double)x_q (dy, dz
 * likewise), (dx*dx + dy*dy) + dz*dz <= radius*radius -- inclusive, IEEE double, that association, no
 * contraction.  Points with equal coordinates are adjacent.  A point of two masks is a node of its own in each:
 * connectivity never passes from one mask to another.
 * COMPONENTS: the connected components of that graph; KEY of a component = its smallest point index, SIZE = its
 * number of points.  SG_SPLIT_ALL: every component with size >= min_npoint is an output.  SG_SPLIT_LARGEST: per
 * mask only the component of greatest size, the smaller key among equal sizes, and only if its size reaches
 * min_npoint.  A mask without a surviving component (an empty one included) yields nothing.
 * OUTPUTS in ascending (source mask, key) order: out_bits uint32 [n_out, ceil(n_points / 32)] (every word written,
 * bits at and beyond n_points zero), source int32 [n_out] = index of the input mask, npoint int32 [n_out].
 * INVALID INPUT: a coordinate of a MASK point (points in no mask are never looked at) that is not finite sets
 * SG_SPLIT_FLAG_NOT_FINITE, one whose cell floor((double)x / radius) reaches 2^31 in magnitude
 * SG_SPLIT_FLAG_CELL_RANGE; the flag is decided by a kernel of its own before any table is touched, and then
 * nothing is labelled and meta[0] = 0.
 * The hashed grid of cells of `radius` is a means: two points within the radius lie at most one cell apart per axis,
 * or two where the quotient of one of them lies within rounding of a cell face, and the walk covers both -- the
 * result equals the brute force over all pairs of a mask for every input.
 *
 * TWO PASSES over one workspace.  sg_mask_split_count writes meta int32 [4] (device): [0] = n_out, [1] = flags,
 * [2] = P = mask points in all = sum of the rows' populations (INT32_MAX when more), [3] = components before the
 * selection (0 with a validity flag).  After one read-back of meta, sg_mask_split_fill (same n_inst, n_points and
 * ws, n_pairs = meta[2]) writes the first `capacity` outputs; it must not be called when meta[1] != 0.
 * WORKSPACE: memory is proportional to P, which only the device knows: sg_mask_split_workspace_bytes(n_inst,
 * n_points, n_pairs) is the size for up to n_pairs mask points (100 - 160 bytes each, and 4 per word of bits).  The
 * count pass first counts P (a prefix over the words) and reads it back -- it synchronises `stream` ONCE -- and
 * when ws_bytes < sg_mask_split_workspace_bytes(n_inst, n_points, P) it returns SG_ERR_WORKSPACE having written
 * nothing beyond the prefix: meta[2] holds P, call again with that size.  It needs at least
 * sg_mask_split_workspace_bytes(n_inst, n_points, 0) to count.
 * RANGE: n_inst <= 16384, n_out <= 16384, n_points < 2^31, P < 2^31.  sg_mask_split_workspace_bytes returns 0 and
 * the calls SG_ERR_UNSUPPORTED outside the range that the host can see (n_inst, n_points, n_pairs; P once counted);
 * more than 16384 outputs set SG_SPLIT_FLAG_TOO_MANY (meta[0] still holds their number, the fill pass then writes
 * nothing) -- nothing is truncated.
 * DETERMINISM: integer atomics only (compare-and-swap on a union-find parent with parent[i] <= i, add on sizes,
 * max on a (size, ~key) word, OR on bits); every order that reaches an output comes from indices: two calls on the
 * same input give the same bytes.  No thread waits for another; every loop has a bound that does not depend on the
 * data beyond P, and a bound that is hit sets SG_SPLIT_FLAG_INTERNAL instead of spinning. */
#define SG_SPLIT_ALL 0
#define SG_SPLIT_LARGEST 1
#define SG_SPLIT_FLAG_NOT_FINITE 1
#define SG_SPLIT_FLAG_CELL_RANGE 2
#define SG_SPLIT_FLAG_INTERNAL 4
#define SG_SPLIT_FLAG_TOO_MANY 8
size_t sg_mask_split_workspace_bytes(int n_inst, int64_t n_points, int64_t n_pairs);
int sg_mask_split_count(const float *xyz, const uint32_t *bits, int n_inst, int64_t n_points, double radius,
                        int min_npoint, int mode, int32_t *meta, void *ws, size_t ws_bytes, sg_stream_t stream);
int sg_mask_split_fill(int n_inst, int64_t n_points, int64_t n_pairs, const void *ws, size_t ws_bytes,
                       int64_t capacity, uint32_t *out_bits, int32_t *source, int32_t *npoint, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Masks and semantic labels snapped to an over-segmentation, "superpoints" (csrc/superpoint.hip).  The reference has
 * NO counterpart; ScanNet ships such a segmentation with every scene (`*.segs.json`) and most pipelines refine their
 * masks and labels on it.  This stage is new and opt-in (softgroup_amd.util.refine_result); nothing calls it unless
 * asked.  softgroup_amd.ops.superpoint's numpy twins are the definition, the kernels equal them byte for byte.
 *
 * IDS: sp int32 [n_points], the superpoint id of every point: arbitrary (not dense, not ordered), anything in
 * 0 .. 2^31 - 2; -1 = in no superpoint.  An id below -1 or equal to 2^31 - 1 sets SG_SUPERPOINT_FLAG_ID; a kernel of
 * its own decides that before anything else runs, and with the flag set nothing but meta is written (meta = [0, flag,
 * 0, 0]).  No id ever addresses memory: ids are sort keys only.
 * SEGMENTS: a segment is the set of points with one id, its size their number.  Segments are numbered 0 .. S-1 in
 * ascending id order; inside a segment the points are in ascending index order.
 * sg_superpoint_index (once per cloud) writes
 *   order     int32 [n_points]      the points of segment 0, then of segment 1, ...; the first n_valid entries
 *   seg_of    int32 [n_points]      the segment of a point, -1 for none (every entry written)
 *   seg_start int32 [n_points + 1]  segment s = order[seg_start[s] .. seg_start[s+1]); the first S + 1 entries
 *   meta      int32 [4]             [S, flags, n_valid, largest segment size]
 * and never synchronises; the caller reads meta back once.
 *
 * MASK SNAP.  bits: the rows of sg_mask_nms, uint32 [n_inst, ceil(n_points / 32)], bits at and beyond n_points
 * ignored.  For mask k and segment s, inter = the points of s in mask k; the segment is TAKEN by the mask when
 * inter >= 1 and (double)inter / (double)size > thr -- strict, one IEEE double division of the two integers; thr a
 * double in [0, 1].  Output bit (k, p): a point in no superpoint keeps its input bit; SG_SNAP_SNAP gives
 * taken(k, seg(p)); SG_SNAP_GROW in | taken (only adds points); SG_SNAP_TRIM in & taken (only removes points).
 * out_bits uint32 [n_inst, ceil(n_points / 32)]: every word written, bits at and beyond n_points zero, rows in the
 * input order, nothing dropped; it must not alias bits.  npoint int32 [n_inst]: the populations of the output rows.
 * order / seg_of / seg_start / n_seg / n_valid: what sg_superpoint_index produced for this cloud.
 * No synchronisation and no read-back.
 *
 * LABEL VOTE.  labels int32 [n_points].  Per segment the points whose label lies in 0 .. n_classes - 1 and differs
 * from ignore_label are counted per class; every other value is not counted.  The winner is the class with the
 * greatest count, the lowest class among equal counts; every point of the segment receives it (also the points that
 * carried an uncounted label).  A segment without a counted label keeps every point's own label, and so do the points
 * in no superpoint.  out_labels int32 [n_points]; seg_label (may be NULL) int32 [n_seg]: the winner, -1 for none.
 *
 * A workgroup walks SG_SUPERPOINT_WALK consecutive positions of `order`; a segment that crosses such a boundary is
 * summed over several workgroups in a global int32 counter (integer adds: no order reaches an output).
 * RANGE: n_inst <= 16384, n_points < 2^31, 1 <= n_classes <= 256.  Outside it the _workspace_bytes functions return 0
 * and the calls SG_ERR_UNSUPPORTED -- nothing is truncated.  Every loop is bounded by sizes the host passed; every
 * index read from order, seg_of or seg_start is range-checked before it addresses anything, so an index array that
 * sg_superpoint_index did not write gives wrong bits but never a read or a write outside the buffers.
 * DETERMINISM: integer adds and ORs only; two calls on the same input give the same bytes. */
#define SG_SNAP_SNAP 0
#define SG_SNAP_GROW 1
#define SG_SNAP_TRIM 2
#define SG_SUPERPOINT_FLAG_ID 1
#define SG_SUPERPOINT_WALK 2048
size_t sg_superpoint_index_workspace_bytes(int64_t n_points);
int sg_superpoint_index(const int32_t *sp, int64_t n_points, int32_t *order, int32_t *seg_of, int32_t *seg_start,
                        int32_t *meta, void *ws, size_t ws_bytes, sg_stream_t stream);
size_t sg_mask_snap_workspace_bytes(int n_inst, int64_t n_points, int64_t n_seg);
int sg_mask_snap(const uint32_t *bits, int n_inst, int64_t n_points, const int32_t *order, const int32_t *seg_of,
                 const int32_t *seg_start, int64_t n_seg, int64_t n_valid, double thr, int mode, uint32_t *out_bits,
                 int32_t *npoint, void *ws, size_t ws_bytes, sg_stream_t stream);
size_t sg_superpoint_vote_workspace_bytes(int64_t n_points, int64_t n_seg, int n_classes);
int sg_superpoint_vote(const int32_t *labels, int64_t n_points, const int32_t *order, const int32_t *seg_of,
                       const int32_t *seg_start, int64_t n_seg, int n_classes, int ignore_label, int32_t *out_labels,
                       int32_t *seg_label, void *ws, size_t ws_bytes, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Native host driver of the grouping head and of the result extraction (csrc/scan_exec.hip): what
 * SoftGroup.forward_grouping + clusters_voxelization (softgroup/model/softgroup.py:411-480,655-709)
 * and get_instances (:537-604) do between the network's dense heads, as one C call each --
 * class selection, ball query, BFS clustering, proposal voxel index and pooled features in the
 * first; kept-instance table, mask runs, RLE text and the copy to the host in the second.  Same
 * kernels as the per-operator entry points above plus fused replacements of the torch glue; same
 * results, bit for bit (every float operation of the glue is the separate IEEE operation torch
 * performs).  Covers the plain SoftGroup path (no pyramid / octree grouping, no lvl_fusion, no
 * sem2ins classes); anything else stays on the per-operator path.
 * Device memory: ONE caller-provided arena per call, carved in call order; results are returned as
 * BYTE OFFSETS into it.  SG_ERR_WORKSPACE + arena_needed (an estimate; retry may ask again) when it
 * is too small.  Both calls synchronise `stream` several times (data-dependent sizes).
 * ---------------------------------------------------------------------------------------- */
typedef struct sg_grouping_cfg {
  int n_points;              /* N */
  int n_sem_classes;         /* columns of `scores` */
  int n_seg;                 /* grouped classes, <= 32 (semantic classes minus ignore_classes) */
  const int32_t *seg_class;  /* device [n_seg], ascending: semantic class of segment s */
  const float *seg_thr;      /* device [n_seg]: npoint_thr, or npoint_thr * class_numpoint_mean (fp32 product) */
  float score_thr;           /* grouping_cfg.score_thr (strict >) */
  int min_npoint;            /* test_cfg.min_npoint: classes with fewer selected points are skipped */
  float radius;              /* grouping_cfg.radius */
  int batch_size;
  float voxel_scale;         /* instance_voxel_cfg.scale */
  int voxel_shape;           /* instance_voxel_cfg.spatial_shape; 0 = stop after the proposals (the
                                training step voxelises them itself, with rand_quantize) */
  int feat_channels;         /* C of point_feats */
} sg_grouping_cfg;
typedef struct sg_grouping_result {   /* host */
  int n_selected, n_neighbours, n_proposals, sum_npoint, n_voxels, max_active;
  size_t proposals_idx;      /* int32 [sum_npoint, 2] = (proposal, scene point) */
  size_t proposals_offset;   /* int32 [n_proposals + 1] */
  size_t voxel_coords;       /* int32 [n_voxels, 4] = (proposal, x, y, z) */
  size_t voxel_offsets;      /* int32 [n_proposals + 1]: first voxel of every proposal */
  size_t voxel_feats;        /* float [n_voxels, C] */
  size_t point_to_voxel;     /* int32 [sum_npoint] */
  size_t arena_used, arena_needed;
  int deferred_classes;      /* sg_scan_grouping_pp: classes whose tail ran behind their giant clusters' replay (0 | 1) */
  int reserved_;
} sg_grouping_result;
/* scores f32 [N, n_sem_classes] = softmax of the semantic logits; pt_offsets, coords_float f32 [N,3];
 * batch_idxs int32 [N]; point_feats f32 [N, C] = backbone features per point. */
int sg_scan_grouping(const sg_grouping_cfg *cfg, const float *scores, const float *pt_offsets,
                     const float *coords_float, const int32_t *batch_idxs, const float *point_feats,
                     void *arena, size_t arena_bytes, sg_grouping_result *result_host,
                     sg_stream_t stream);

/* SoftGroup++ grouping (softgroup/model/softgroup.py:433-466 with with_pyramid / with_octree; per-class level
 * get_level :485-489, pyramid_map :491-498, octree query softgroup/ops/functions.py:14-44, bfs_cluster :278-308,
 * pyramid_inverse_map :500-507) as ONE C call: class selection of all classes at once (one read-back of the
 * per-class counts), then class by class on the operators above -- level voxels and their pooled coordinates /
 * offsets, octree or hashed-grid neighbour lists at radius * level, clusters, inverse map -- and the same
 * proposal voxelisation as sg_scan_grouping.  base.radius is ignored: `radius` and `base_size` are the
 * configuration's Python floats (the level's radius and voxel size are their double products rounded once,
 * as the reference's Python computes them).  Same results as the per-class loop over the operator surface,
 * bit for bit.  2 + 4 host read-backs per grouped class (voxel count, neighbour total, cluster count, rows).
 * A class with a cluster above 16 384 points (its ordered emission is a multi-workgroup replay of milliseconds
 * on a side stream) does not hold up the classes behind it: the rest of that class is queued behind the replay,
 * the next classes run next to it, one join before the proposals are voxelised (result->deferred_classes). */
typedef struct sg_grouping_pp_cfg {
  sg_grouping_cfg base;
  int with_pyramid, with_octree, lvl_fusion;
  double radius;             /* grouping_cfg.radius */
  double base_size;          /* grouping_cfg.pyramid_base_size */
} sg_grouping_pp_cfg;
int sg_scan_grouping_pp(const sg_grouping_pp_cfg *cfg, const float *scores, const float *pt_offsets,
                        const float *coords_float, const int32_t *batch_idxs, const float *point_feats,
                        void *arena, size_t arena_bytes, sg_grouping_result *result_host,
                        sg_stream_t stream);

/* Host-side staging copies of the device-side collate (the reference's collate_fn, data/custom.py:196-256, does
 * them with torch.cat on the CPU): dense / strided row copies, the float64 -> float32 cast of an item's labels and
 * the batch-index column of the collated coordinates, as plain C so that a binding can run them without the
 * interpreter lock (a loader thread preparing the next scan next to the threads that drive the scans in flight). */
int sg_host_copy_2d(void *dst, int64_t dst_pitch_bytes, const void *src, int64_t src_pitch_bytes, int64_t rows,
                    int64_t row_bytes);
int sg_host_cast_f64_f32(float *dst, const double *src, int64_t n);
int sg_host_fill_i64_strided(int64_t *dst, int64_t pitch_elems, int64_t rows, int64_t value);
/* out_max[c] = max over the rows of src[r * cols + c] (INT64_MIN for no rows), cols <= 8: the collate's
 * spatial_shape (data/custom.py:246) without numpy's 1.3 ms axis-0 reduction under the interpreter lock */
int sg_host_colmax_i64(const int64_t *src, int64_t rows, int64_t cols, int64_t *out_max);

typedef struct sg_instances_cfg {
  int n_proposals, n_classes;   /* instance classes (without the background column) */
  int score_stride;             /* columns of cls_prob / iou_scores / mask_scores (n_classes + 1) */
  int64_t sum_npoint;           /* rows of proposals_idx / mask_scores */
  int n_points;                 /* mask length N */
  float cls_score_thr, mask_score_thr;
  int min_npoint;
} sg_instances_cfg;
typedef struct sg_instances_result {   /* host */
  int n_kept;
  size_t off_class, off_score, off_text, text_bytes;   /* byte offsets into host_out */
  size_t host_needed, arena_used, arena_needed;
  size_t bits;        /* arena offset: uint32 [n_kept, ceil(n_points / 32)] bit rows of the kept masks */
  size_t label_id;    /* arena offset: int32 [n_kept] (device copy of the labels) */
} sg_instances_result;
/* proposals_idx int32 [S,2]; mask_scores f32 [S, stride] (per pair); cls_prob f32 [nP, stride] =
 * softmax of the class logits; iou_scores f32 [nP, stride].  host_out (pinned host memory) receives
 *   int64 text_off[n_kept + 1] | int32 label_id[n_kept] at off_class | f32 conf[n_kept] at off_score
 *   | the RLE text at off_text: instance k's "start len ..." string is
 *   text[text_off[k] .. text_off[k+1] - 1) (sg_rle_format_device's convention).
 * Instances come in the reference's order (class-major, proposal-ascending, softgroup.py:566-603). */
int sg_scan_instances(const sg_instances_cfg *cfg, const int32_t *proposals_idx, const float *mask_scores,
                      const float *cls_prob, const float *iou_scores, void *arena, size_t arena_bytes,
                      void *host_out, size_t host_bytes, sg_instances_result *result_host,
                      sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * One scan = one call (csrc/scan_forward.hip): the whole of SoftGroup.forward_test
 * (softgroup/model/softgroup.py:299-361) for the instance-segmentation configurations (SoftGroup, and SoftGroup++
 * through desc->with_pyramid / with_octree; not panoptic fusion, lvl_fusion or x4_split) -- voxel feature pooling
 * (:305), backbone (:307-309 -> forward_backbone :363-378), point-wise heads + arg-max, softmax of the
 * semantic scores, grouping head and proposal voxelisation (:411-480, :655-709), tiny U-Net (:671-675),
 * mask / class / IoU heads (:676-686), instance extraction + RLE text (:537-604) and the dense per-point
 * results of get_point_wise_results / get_gt_instances (:641-653) -- chained on the caller's stream with
 * nothing but kernel launches and the data-dependent read-backs in between.  The reference runs one scan
 * per process at a time from its test loop (tools/test.py:145-150); a host thread that makes this ONE call
 * holds no interpreter lock while the scan runs.  Same kernels and entry points as the calls above
 * (sg_voxelize_fp's arithmetic, sg_unet_forward, sg_pointwise_heads, sg_scan_grouping, sg_scan_instances);
 * the dense heads of the refinement (nn.Linear / MLP on <= a few thousand rows) are fp32 FMA chains in
 * ascending channel order like sg_pointwise_heads.
 *   arena: device scratch, carved in call order; SG_ERR_WORKSPACE + result->arena_needed when too small.
 *   host_dense / host_inst: PINNED host memory for the dense results and for sg_scan_instances' image.
 * ---------------------------------------------------------------------------------------- */
typedef struct sg_linear {            /* nn.Linear: w [out][in], b [out] */
  const float *w, *b;
  int out, in;
} sg_linear;
/* row-wise softmax with torch's arithmetic for rows of <= 32 columns (softmax_warp_forward: maximum,
 * exp(x - max) by expf, the sum as a 32-lane butterfly -- offsets 16, 8, 4, 2, 1 -- and one division per
 * element): bit-identical to tensor.softmax(-1) on this build (tests/test_scan_forward_gpu.py) */
int sg_softmax_rows(const float *x, int64_t rows, int cols, float *out, sg_stream_t stream);
/* out[r, :] = mlp(feats[idx[r], :]) (idx NULL: identity); channels 16 or 32, mlp->out <= 32 */
int sg_mlp_rows(const float *feats, const int32_t *idx, int64_t rows, int channels, const sg_mlp2 *mlp,
                float *out, sg_stream_t stream);
/* out[r, j] = b[j] + sum_c x[r, c] * w[j, c], ascending c (fmaf chain) */
int sg_linear_rows(const float *x, int64_t rows, const sg_linear *lin, float *out, sg_stream_t stream);

#define SG_SCAN_DENSE_MAX 16
typedef struct sg_scan_dense_item {
  int kind;            /* 0 = `ptr`/`bytes` (a device buffer passed through to the host block),
                          1 = semantic_preds int64 [N], 2 = offset_preds f32 [N,3],
                          3 = gt_instances int64 [N] (softgroup.py:641-653 from semantic_labels / instance_labels),
                          4 = semantic_scores f32 [N, n_sem] (the logits) */
  const void *ptr;
  size_t bytes;
} sg_scan_dense_item;
typedef struct sg_scan_desc {
  const sg_unet_desc *backbone;       /* input_conv + unet + output_layer */
  const sg_unet_desc *tiny;           /* tiny_unet + tiny_unet_outputlayer */
  sg_mlp2 semantic, offset, mask;     /* semantic_linear, offset_linear, mask_linear */
  sg_linear cls, iou;                 /* cls_linear, iou_score_linear */
  int channels;                       /* backbone output channels: 16 or 32 */
  int with_coords;                    /* voxel features = [feats | coords_float] */
  int semantic_classes, instance_classes;
  sg_grouping_cfg grouping;           /* n_points / batch_size / feat_channels are filled per call */
  float cls_score_thr, mask_score_thr;
  int min_npoint;
  int want_instances;                 /* 0: stop after the point-wise heads */
  /* SoftGroup++ grouping (sg_scan_grouping_pp instead of sg_scan_grouping) when either switch is set; pp_radius /
   * pp_base_size are the configuration's Python floats (grouping_cfg.radius, .pyramid_base_size) */
  int with_pyramid, with_octree;
  double pp_radius, pp_base_size;
} sg_scan_desc;
typedef struct sg_scan_input {        /* one collated batch, device pointers (data/custom.py:240-256) */
  int n_points, n_voxels, max_active; /* p2v_map is int32 [n_voxels, 1 + max_active] */
  int batch_size;
  int spatial_shape[3];
  const float *feats;                 /* f32 [N, feat_dim] */
  int feat_dim;
  const float *coords_float;          /* f32 [N, 3] */
  const int32_t *p2v_map;
  const void *v2p_map;                /* [N] int32 or int64 */
  int v2p_is_int64;
  const void *voxel_coords;           /* [M, 4] int32 or int64 */
  int voxel_coords_is_int64;
  const int32_t *batch_idxs;          /* int32 [N] */
  const int64_t *semantic_labels, *instance_labels;   /* for dense kind 3 (may be NULL) */
  int n_dense;
  sg_scan_dense_item dense[SG_SCAN_DENSE_MAX];
} sg_scan_input;
typedef struct sg_scan_result {       /* host */
  sg_grouping_result grouping;        /* counts; its offsets are relative to `grouping_base` */
  sg_instances_result instances;      /* offsets into host_inst / relative to `instances_base` */
  size_t grouping_base, instances_base;               /* arena offsets of the two stages' sub-arenas */
  size_t dense_offset[SG_SCAN_DENSE_MAX];             /* byte offsets into host_dense */
  size_t dense_bytes;                                 /* bytes of host_dense in use */
  /* arena offsets of the stage outputs (device; valid until the next call on this arena) */
  size_t voxel_feats_in, backbone_out, output_feats, semantic_scores, semantic_prob, pt_offsets,
      semantic_preds, tiny_out, mask_scores, cls_scores, cls_prob, iou_scores;
  size_t arena_used, arena_needed, host_dense_needed, host_inst_needed;
  int stage;                          /* how far the call got: 1 heads, 2 grouping, 3 refinement, 4 instances */
} sg_scan_result;
size_t sg_scan_arena_bytes(const sg_scan_desc *desc, int n_points, int n_voxels);
int sg_scan_forward(const sg_scan_desc *desc, const sg_scan_input *in, void *arena, size_t arena_bytes,
                    void *host_dense, size_t host_dense_bytes, void *host_inst, size_t host_inst_bytes,
                    sg_scan_result *result_host, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation (ScanNetEval.assign_instances_for_scan, softgroup/evaluation/instance_eval.py:228-309):
 * counts[p*n_slots + s] = number of points of prediction p's mask whose ground-truth slot is s.
 * Masks come as runs: run r covers points run_start[r] .. run_start[r] + len(r) - 1 of prediction
 * run_pred[r]; run_off[r] = sum of the lengths of runs < r (run_off[n_runs] = total_points).
 * gt_slot[point] in [0, n_slots): index of the point's GT instance, n_slots-1 = void.
 * ---------------------------------------------------------------------------------------- */
int sg_eval_intersections(const int32_t *run_start, const int64_t *run_off, const int32_t *run_pred,
                          int n_runs, int64_t total_points, const int32_t *gt_slot, int n_pred,
                          int n_slots, int32_t *counts, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Point-wise and panoptic evaluation.  Label arrays are typed by a kind: SG_EVAL_I32, SG_EVAL_I64
 * or SG_EVAL_U32 (int32 storage read as unsigned), each buffer 16-byte aligned; offsets are
 * float32 [n, 3].  Outputs accumulate (the caller zeroes them once), so chunks of scans add up.
 * *flags gets SG_EVAL_BAD_* bits for inputs the kernels cannot represent exactly; the caller then
 * evaluates on the host.
 * ---------------------------------------------------------------------------------------- */
#define SG_EVAL_I32 0
#define SG_EVAL_I64 1
#define SG_EVAL_U32 2
#define SG_EVAL_MAX_CLASSES 1024
#define SG_EVAL_BAD_GT 1      /* a valid gt class outside [0, n_classes) */
#define SG_EVAL_BAD_PRED 2    /* panoptic: a prediction outside [0, 2**32) */
#define SG_EVAL_BAD_INST 4    /* panoptic: an instance label whose y_inst does not fit 31 bits */

/* evaluate_semantic_acc / evaluate_semantic_miou / evaluate_offset_mae
 * (softgroup/evaluation/point_wise_eval.py:4-44) and PanopticEval's seen / correct / positive
 * (softgroup/evaluation/panoptic_eval.py:58-62): over the points with gt != ignore_label,
 *   tallies[c] += seen, tallies[n_classes + c] += positive, tallies[2 n_classes + c] += correct
 * (pred class = pred, or pred & 0xFFFF when `panoptic`; predictions outside [0, n_classes) count
 * nowhere).  With offset_pred non-null also, over the points with inst != ignore_label,
 *   *offset_sum += sum of |offset_gt - offset_pred| (float32 differences, fp64 sum in a fixed
 *   order: bitwise repeatable), *offset_count += number of those points.
 * pred NULL: offsets only (gt and tallies unused).
 * ws: sg_eval_tally_workspace_bytes(n_points) bytes (only used with offsets). */
size_t sg_eval_tally_workspace_bytes(int64_t n_points);
int sg_eval_class_tally(const void *pred, int pred_kind, const void *gt, int gt_kind, int64_t n_points,
                        int64_t ignore_label, int panoptic, int n_classes, uint64_t *tallies,
                        const void *inst, int inst_kind, const float *offset_pred, const float *offset_gt,
                        double *offset_sum, uint64_t *offset_count, int32_t *flags, void *ws, size_t ws_bytes,
                        sg_stream_t stream);

/* PanopticEval.evaluate_single's segment matching (softgroup/evaluation/panoptic_eval.py:24-166)
 * for n_scans scans laid end to end (scan s = points scan_off[s] .. scan_off[s+1]-1, n_scans <=
 * 65535, n_points < 2**30).  Over the points with sem != ignore_label: pred segments (scan, pred & 0xFFFF,
 * pred + 1), gt segments (scan, sem, y) with y = (inst == ignore_label ? -1 : inst) + 2 > 0, and their
 * intersections.  A pair with I / U > 0.5 (double) is a TP: its row (scan << 16 | cl, y << 32 | x,
 * I, U) goes to tp_rows[4 * r] (capacity n_points rows); *tp_count is set to the number of rows.
 * Unmatched segments of at least min_points points add to fp_fn[cl] (pred) and fp_fn[n_classes + cl]
 * (gt).
 * ws: sg_eval_panoptic_workspace_bytes(n_points) bytes. */
size_t sg_eval_panoptic_workspace_bytes(int64_t n_points);
int sg_eval_panoptic_segments(const void *pred, int pred_kind, const void *sem, int sem_kind,
                              const void *inst, int inst_kind, const int64_t *scan_off, int n_scans,
                              int64_t n_points, int64_t ignore_label, int n_classes, int64_t min_points,
                              uint64_t *fp_fn, int64_t *tp_rows, uint64_t *tp_count, int32_t *flags,
                              void *ws, size_t ws_bytes, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * ScanNetEval on the device (softgroup/evaluation/instance_eval.py, instance_eval_util.py's
 * get_instances): per scan RLE text -> runs -> GT table -> intersections -> pair records -> greedy
 * matching, examples appended to a device-resident accumulator; then the curves of all
 * (label, threshold) segments at once.  *flags gets SG_INST_* bits; nothing is truncated silently.
 * ---------------------------------------------------------------------------------------- */
#define SG_INST_BAD_TEXT 1       /* RLE text: a byte that is neither a digit nor white space */
#define SG_INST_ODD_TOKENS 2     /* RLE text: an odd number of tokens */
#define SG_INST_RUN_RANGE 4      /* RLE text: a run outside [0, length), or more mask points than points */
#define SG_INST_BAD_GT 8         /* a gt id below 0 or >= 2**31 */
#define SG_INST_OVERFLOW_GT 16   /* more GT instances in a scan than gt_cap */
#define SG_INST_OVERFLOW_EX 32   /* more examples than ex_cap (totals[0] = the number needed so far) */
#define SG_INST_NO_EXAMPLES 64   /* a label with GT and predictions but no example: the reference raises IndexError */
#define SG_INST_MAX_THRESHOLDS 16
#define SG_INST_SECTIONS 16

/* rle_decode's text split (softgroup/util/rle.py:25-36, instance_eval.py:377) for n_masks masks of one
 * scan: text = the masks' `counts` strings laid end to end, mask m = bytes text_off[m] .. text_off[m+1]-1
 * (device int64 [n_masks + 1], text_off[n_masks] <= text_bytes).  Mask m's runs go to the slots from
 * (text_off[m] + m) / 4 on, 0-based: run_start, run_len, run_pred = mask_pred[m] (m when NULL); slots
 * without a run have length 0; run_slots >= sg_inst_rle_run_slots(text_bytes, n_masks), else
 * SG_ERR_WORKSPACE.  vert_count[mask_pred[m]] = the mask's points.  A run that fails its check is emptied. */
int64_t sg_inst_rle_run_slots(int64_t text_bytes, int n_masks);
int sg_inst_rle_parse(const uint8_t *text, const int64_t *text_off, const int32_t *mask_pred, int n_masks,
                      int64_t text_bytes, int64_t length, int32_t *run_start, int32_t *run_len, int32_t *run_pred,
                      int64_t run_slots, int32_t *vert_count, int32_t *flags, sg_stream_t stream);

/* One scan (get_instances; assign_instances_for_scan :228-309; evaluate_matches :82-139).  gts: int64 ids
 * class * 1000 + instance.  Runs as above (slots of length 0 allowed).  pred_label[p] = evaluated label
 * index or -1 (not evaluated), pred_vert, pred_conf (finite, no -0.0) per prediction in list order; a
 * prediction takes part when its label >= 0 and pred_vert >= min_region.  n_labels = n_classes, or 1 for the
 * class-agnostic form.  thresholds: host doubles, n_thr <= SG_INST_MAX_THRESHOLDS.
 * Appends (order-preserving score key, segment << 1 | true) examples, segment = label * n_thr + threshold,
 * at totals[0] (device int64, zero at the start of an evaluation) and adds to seg_stats [4][n_labels * n_thr]
 * (examples, hard false negatives, has_gt, has_pred; zero at the start).
 * ws: sg_inst_scan_workspace_bytes bytes (0 = arguments out of range: n_pred * n_points < 2**31,
 * n_pred * (gt_cap + 1) < 2**28); section_off (host, SG_INST_SECTIONS entries, may be NULL) receives the byte
 * offsets of the scan's tables inside ws: 0 info int32 [8] (n_gt, mask points, pairs), 1-3 gt_id / gt_label /
 * gt_vert int32 [gt_cap], 4 gt_pair_off [gt_cap + 1], 5 pred_pair_off [n_pred + 1], 6 pred_void [n_pred],
 * 7-10 pairs by GT then prediction (gt, pred, inter int32; iou double), 11-14 the same by prediction then GT,
 * 15 counts int32 [n_pred][gt_cap + 1] (last column: void). */
size_t sg_inst_scan_workspace_bytes(int64_t n_points, int n_pred, int64_t run_slots, int n_classes, int gt_cap,
                                    int n_thr, int n_labels, int64_t *section_off);
int sg_inst_scan_update(const int64_t *gts, int64_t n_points, const int32_t *run_start, const int32_t *run_len,
                        const int32_t *run_pred, int64_t run_slots, const int32_t *pred_label,
                        const int32_t *pred_vert, const double *pred_conf, int n_pred, int n_labels, int n_classes,
                        int64_t min_region, const double *thresholds, int n_thr, int gt_cap, uint64_t *ex_key,
                        uint32_t *ex_meta, int64_t ex_cap, int32_t *seg_stats, int64_t *totals, int32_t *flags,
                        void *ws, size_t ws_bytes, sg_stream_t stream);

/* S3DIS coverage / precision / recall of the scan that the last sg_inst_scan_update left in ws (same sizing
 * arguments, same layout; enqueue it right behind that call, on the same stream).  The reference has no code
 * for these; the definitions, per scan and evaluated label l:
 *   GT instances of l: every row of the scan's GT table with that label, ascending id, all sizes.
 *   participating predictions: label >= 0, pred_vert >= min_region and pred_conf >= score_thr.
 *   ov_gt(g)   = max IoU over the participating predictions of l (0.0 without any); ov_pred(p) = max IoU over
 *                the GT instances of l (0.0 without any); IoU = inter / (gt_vert + pred_vert - inter) in double,
 *                as the pair records hold it (same label, inter > 0).
 *   cov  = (sum_g ov_gt(g)) / n_gt,  wcov = (sum_g ov_gt(g) * vert(g)) / sum_g vert(g), both only when n_gt > 0
 *          (the scan is then a "room" of l); gt_hit = GTs with ov_gt >= iou_thr; a participating prediction is a
 *          tp when ov_pred >= iou_thr, else an fp.
 * Reads from ws: info (n_gt, pairs), gt_label, gt_vert, gt_pair_off, pred_pair_off, the pred and iou columns of
 * the pairs by GT and the iou column of the pairs by prediction.  One workgroup per label: the maxima in
 * parallel, then one lane sums over ascending GT id with a rounded multiply and rounded adds (no fused
 * multiply-add) and adds to cov_sums (device double [2][n_labels]: cov, wcov) and tallies (device int64
 * [5][n_labels]: rooms, n_gt, gt_hit, tp, fp), both zero at the start of an evaluation.  No floating-point
 * atomics: bitwise repeatable, and equal to the host evaluator's sums.  A scan behind a non-zero *flags adds
 * nothing (that evaluation is redone or handed to the host); table entries are clamped to gt_cap, n_pred and
 * the pair capacity before anything is indexed. */
int sg_inst_scan_coverage(int64_t n_points, int n_pred, int64_t run_slots, int n_classes, int gt_cap, int n_thr,
                          int n_labels, const int32_t *pred_label, const int32_t *pred_vert,
                          const double *pred_conf, int64_t min_region, double iou_thr, double score_thr,
                          double *cov_sums, int64_t *tallies, const int32_t *flags, void *ws, size_t ws_bytes,
                          sg_stream_t stream);

/* The curves (evaluate_matches :146-199): the examples sorted by (segment, score), cumulative true count,
 * np.unique's boundaries, precision / recall in double, AP summed in a fixed order -> ap, rc [n_seg]
 * (0.0 for a segment with GT only, NaN without GT).  ws: sg_inst_curves_workspace_bytes bytes. */
size_t sg_inst_curves_workspace_bytes(int64_t n_examples, int n_seg);
int sg_inst_curves(const uint64_t *ex_key, const uint32_t *ex_meta, int64_t n_examples, const int32_t *seg_stats,
                   int n_seg, double *ap, double *rc, int32_t *flags, void *ws, size_t ws_bytes,
                   sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Axis-aligned box detection AP (tools/eval_det.py).  Coordinates are [n, 3] row-major, float32
 * (coords_f64 = 0) or float64 (1), of all scans laid end to end.  boxes[6 o .. 6 o + 5] = (xmin ymin
 * zmin xmax ymax zmax) of owner o in float64, exact (order-preserving integer keys); an owner without
 * points gets NaN.  *flags gets SG_DET_BAD_COORD when an owned point has a non-finite coordinate
 * (the caller then forms the boxes on the host: numpy's min / max propagate NaN).
 * ---------------------------------------------------------------------------------------- */
#define SG_DET_BAD_COORD 1
#define SG_DET_MAX_THRESHOLDS 16

/* Prediction boxes, coords[mask].min(0) / .max(0) (eval_det.py:290-297).  Masks come as runs, as for
 * sg_eval_intersections: run r covers points run_start[r] .. run_start[r] + len(r) - 1 (global point
 * indices) of owner run_owner[r] in [0, n_owner); run_off = exclusive prefix sum of the lengths
 * (run_off[n_runs] = total_points). */
int sg_det_boxes_runs(const void *coords, int coords_f64, const int64_t *run_start, const int64_t *run_off,
                      const int32_t *run_owner, int64_t n_runs, int64_t total_points, int64_t n_owner,
                      double *boxes, int32_t *flags, sg_stream_t stream);

/* GT instance boxes, coords[instance_label == i].min(0) / .max(0) (eval_det.py:301-313), for n_scans
 * scans (scan s = points scan_off[s] .. scan_off[s+1]-1): a point of scan s with label l in
 * [0, owner_off[s+1] - owner_off[s]) belongs to owner owner_off[s] + l; other labels (-100) are
 * ignored.  count[o] = points of owner o; first[o] = its lowest global point index, -1 without points
 * (the reference takes the class from semantic_label[np.nonzero(inds)[0][0]]). */
int sg_det_boxes_labels(const void *coords, int coords_f64, const int64_t *labels, const int64_t *scan_off,
                        const int64_t *owner_off, int n_scans, int64_t n_points, int64_t n_owner, double *boxes,
                        int64_t *count, int64_t *first, int32_t *flags, sg_stream_t stream);

/* eval_det_cls's matching (eval_det.py:44-66, 116-146) for every class at once.  Detection d (box
 * det_box[6 d], fp64) belongs to group det_group[d] = one (class, image); the group's GT boxes are
 * gt_box rows group_off[g] .. group_off[g+1]-1.  det_rank[d] = d's position in its class's sorted
 * order (host argsort).  Out: ovmax[d], jmax[d] = the first GT of the group with the strictly largest
 * get_iou (-inf / -1 without one), and tp[k * n_det + d] = 1 when ovmax > thresholds[k] (host array,
 * n_thresholds <= SG_DET_MAX_THRESHOLDS) and d has the lowest rank among the detections with that
 * jmax and ovmax > thresholds[k] -- the greedy pass's TP.  ws: sg_det_match_workspace_bytes bytes. */
size_t sg_det_match_workspace_bytes(int64_t n_gt, int n_thresholds);
int sg_det_match(const double *det_box, const int32_t *det_group, const int32_t *det_rank, int64_t n_det,
                 const double *gt_box, const int64_t *group_off, int64_t n_gt, const double *thresholds,
                 int n_thresholds, double *ovmax, int64_t *jmax, uint8_t *tp, void *ws, size_t ws_bytes,
                 sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Yaw-oriented 3D boxes against each other (csrc/box_ops.hip): the IoU matrix, eval_det_cls's matching with that IoU
 * and greedy box NMS.  The reference has no counterpart.  Opt-in: nothing calls it unless asked.
 * softgroup_amd.ops.boxes.obb_iou_pair is the definition (box_iou_numpy its vectorised twin); every entry equals it
 * byte for byte, and two calls give the same bytes.  Every operation below is ONE IEEE double operation, in the
 * association written, without contraction; the device evaluates no transcendental function; no float atomics.
 *
 * BOX ROW.  8 doubles (cx, cy, cz, du, dv, dz, c, s): du lies along (c, s), dv along (-s, c), (c, s) = (cos theta, sin
 * theta) computed once on the host for both backends (softgroup_amd.ops.boxes.boxes8).  A row with an entry that is
 * not finite or with a negative extent is INVALID: it sets SG_BOX_FLAG_INVALID in the entry's flag word, and the
 * outputs then mean nothing.  No kernel depends on a box being valid in order to terminate or to stay inside its
 * arrays: every loop has a constant bound and every polygon store a slot below 8.
 *
 * AREA(a, b), rectangle a clipped in b's frame (the arguments are not interchangeable at the last bit).
 *   1. hua = 0.5 du_a, hva = 0.5 dv_a.
 *   2. corners k = 0 .. 3, signs (su, sv) = (-,-), (+,-), (+,+), (-,+): u = su hua, v = sv hva,
 *      x = cx_a + (u c_a - v s_a), y = cy_a + (u s_a + v c_a).
 *   3. dx = x - cx_b, dy = y - cy_b, p = (dx c_b + dy s_b, dy c_b - dx s_b).
 *   4. Sutherland-Hodgman against (axis 0, +, hub), (axis 0, -, hub), (axis 1, +, hvb), (axis 1, -, hvb), hub = 0.5
 *      du_b, hvb = 0.5 dv_b.  For the edges (P[i], P[(i + 1) % n]), i ascending: dp = h - sign p[axis], dq likewise; a
 *      vertex is inside when d >= 0 (inclusive; a NaN is outside); p is emitted when inside; when exactly one end is
 *      inside r is emitted as well, t = dp / (dp - dq) (not 0: the signs differ), every coordinate p_k + t (q_k -
 *      p_k), the clipped coordinate then set to exactly sign h.  An empty polygon ends the walk with area 0.  A
 *      convex polygon gains at most one vertex per plane, so 8 slots hold it; an emit into a full polygon is dropped
 *      (never reached by valid boxes).
 *   5. fewer than 3 vertices: area 0.
 *   6. S = +0.0; for i = 1 .. n-2 ascending S = S + ((x_i - x0)(y_{i+1} - y0) - (x_{i+1} - x0)(y_i - y0)); area = 0.5
 *      |S|.
 * IOU, SG_BOX_IOU_3D.  zlo = max(cz_a - 0.5 dz_a, cz_b - 0.5 dz_b), zhi = min(cz_a + 0.5 dz_a, cz_b + 0.5 dz_b) (max(x,
 * y) = x > y ? x : y, min(x, y) = x < y ? x : y), h = zhi - zlo; when h > 0 is false the IoU is 0.0, decided before
 * any clipping.  A = area(a, b); when A > 0 is false the IoU is 0.0.  inter = A h, va = (du_a dv_a) dz_a, vb
 * likewise, uni = (va + vb) - inter; when uni > 0 is false the IoU is 0.0, else inter / uni.  SG_BOX_IOU_BEV: the same
 * without z, uni = (du_a dv_a + du_b dv_b) - A.  Not clamped: a box against itself gives 1 within a few ulps.
 * Touching boxes and boxes of zero extent give exactly 0.  Thresholds compare strictly: iou > thr.
 *
 * sg_box_iou: iou[i n_b + j] = iou(a_i, b_j).  RANGE: 0 <= n_a, n_b and n_a n_b <= 2^30, else SG_ERR_UNSUPPORTED,
 * nothing is launched and nothing truncated.  flags int32 [1] (device, zeroed by the caller) gets
 * SG_BOX_FLAG_INVALID. */
#define SG_BOX_IOU_3D 0
#define SG_BOX_IOU_BEV 1
#define SG_BOX_FLAG_INVALID 1
int sg_box_iou(const double *a, int64_t n_a, const double *b, int64_t n_b, int mode, double *iou, int32_t *flags,
               sg_stream_t stream);

/* sg_det_match with box rows of 8 doubles and the IoU above (mode = SG_BOX_IOU_*): ovmax[d], jmax[d] = the first GT
 * of detection d's (class, image) group with the strictly largest IoU (-inf / -1 without one); the claims are
 * resolved by rank and threshold exactly as sg_det_match does.  The host validates the boxes (there is no flag
 * word).  RANGE: n_det, n_gt < 2^31, 1 <= n_thresholds <= SG_DET_MAX_THRESHOLDS (else SG_ERR_ARG). */
size_t sg_det_match_obb_workspace_bytes(int64_t n_gt, int n_thresholds);
int sg_det_match_obb(const double *det_box, const int32_t *det_group, const int32_t *det_rank, int64_t n_det,
                     const double *gt_box, const int64_t *group_off, int64_t n_gt, const double *thresholds,
                     int n_thresholds, int mode, double *ovmax, int64_t *jmax, uint8_t *tp, void *ws, size_t ws_bytes,
                     sg_stream_t stream);

/* Greedy box NMS: the ORDER and the LOOP of sg_mask_nms, read with iou > thr.  boxes: box rows [n]; scores float32
 * [n], all finite; labels int32 [n], NULL = class-agnostic (as class_agnostic != 0).  Descending score, the LOWER
 * index first among equal scores (-0.0 equals 0.0); a kept box suppresses every later, not yet suppressed box of its
 * label with iou > thr; a suppressed box suppresses nobody.  The pair of original indices i < j is evaluated as
 * iou(box_i, box_j), so the value does not depend on the scores.  keep uint8 [n] (1 = kept) in the original order;
 * n_keep int32 [2] (device): [0] = their number, [1] = the flag word (SG_BOX_FLAG_INVALID; written by the entry).
 * iou_out (may be NULL): double [n, n], [i, j] = [j, i] = iou(box_i, box_j) for i <= j, every pair whatever the labels.
 * RANGE: 0 <= n <= 16384; beyond it the call returns SG_ERR_UNSUPPORTED and sg_box_nms_workspace_bytes returns 0 --
 * nothing is truncated.  Nothing synchronises, there is no host read-back and no float atomic (the decide matrix is
 * set by integer atomicOr). */
size_t sg_box_nms_workspace_bytes(int n);
int sg_box_nms(const double *boxes, int n, const float *scores, const int32_t *labels, double thr, int mode,
               int class_agnostic, uint8_t *keep, int32_t *n_keep, double *iou_out, void *ws, size_t ws_bytes,
               sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training-time data transform (softgroup/data/custom.py:52-194, data/kitti.py:78-118,
 * data/s3dis.py:31-41).  Points are [n, 3] row-major; labels int64.  `stats` receives 9 uint64
 * order-preserving keys of float64 values -- max |x|, min x, max x per axis -- decoded by the caller
 * (key with the top bit set: bits = key ^ 2^63; otherwise bits = ~key).
 * ---------------------------------------------------------------------------------------- */
/* dataAugment's product (custom.py:92-111): xyz_middle = (float32(xyz * scale_factor) if has_scale) @ m
 * in float64 (m_host: 9 doubles, row-major, read on the host); work = xyz_middle * work_scale (/ down
 * when down != 1: kitti.py:96); stats of work. */
int sg_train_augment(const float *xyz, int64_t n, int has_scale, float scale_factor, const double *m_host,
                     double work_scale, double down, double *xyz_middle, double *work, uint64_t *stats,
                     sg_stream_t stream);
/* elastic's six scipy.ndimage.convolve passes with the [1,1,1]/3 box along x, y, z, x, y, z, zero
 * boundary (custom.py:53-64), on n_grids float32 grids [b0, b1, b2] laid end to end, in place (tmp: the
 * same size); each pass sums in float64 and rounds to float32. */
int sg_train_blur(float *grids, float *tmp, int b0, int b1, int b2, int n_grids, sg_stream_t stream);
/* elastic's interpolation and update (custom.py:65-74): work += g(work) * mag, g = trilinear sampling in
 * float64 of the three blurred grids on the axes linspace(-(b-1) gran, (b-1) gran, b), 0 outside, as
 * scipy's RegularGridInterpolator sums it; stats of the result. */
int sg_train_elastic(double *work, int64_t n, const float *grids, int b0, int b1, int b2, double gran, double mag,
                     uint64_t *stats, sg_stream_t stream);
/* crop's test (custom.py:113-127) for k <= 16 candidates cand_host[6 j ..] = (offset xyz, spatial shape
 * xyz): counts[j] = #points p with t + offset >= 0 and < shape on every axis, t = (work * down) - min
 * (min_host: 3 doubles; custom.py:143, kitti.py:101-103). */
int sg_train_crop_count(const double *work, int64_t n, double down, const double *min_host,
                        const double *cand_host, int k, uint64_t *counts, sg_stream_t stream);
/* The kept points in order (custom.py:155-160, 184): coord = trunc(t + offset) (t as above; every point
 * kept and no offset when crop_host is NULL), xyz_middle, feat [n, c] + noise[c] (float32; noise may be
 * NULL), semantic and instance labels; at most out_cap rows are written.  *kept = number of kept points.
 * ws: sg_train_compact_workspace_bytes(n) bytes. */
size_t sg_train_compact_workspace_bytes(int64_t n);
int sg_train_compact(const double *work, const double *xyz_middle, const float *feat, int c, const float *noise,
                     const int64_t *sem, const int64_t *inst, int64_t n, double down, const double *min_host,
                     const double *crop_host, int64_t out_cap, int64_t *coord, double *xyz_middle_out,
                     float *feat_out, int64_t *sem_out, int64_t *inst_out, int32_t *kept, void *ws,
                     size_t ws_bytes, sg_stream_t stream);
/* S3DISDataset.load's subsample (s3dis.py:31-41): rows idx[0..m) of xyz (float32 [n, 3]), feat
 * (float32 [n, c]) and the labels. */
int sg_train_gather(const int64_t *idx, int64_t m, const float *xyz, const float *feat, int c, const int64_t *sem,
                    const int64_t *inst, float *xyz_out, float *feat_out, int64_t *sem_out, int64_t *inst_out,
                    sg_stream_t stream);
/* The set of instance ids present (getCroppedInstLabel, custom.py:129-136 / kitti.py:78-90): labels !=
 * ignore, each once, to out[1 ..] in no particular order, their number to out[0] (only the first cap
 * are stored; cap <= 8192).  ws: sg_train_id_set_workspace_bytes() bytes. */
size_t sg_train_id_set_workspace_bytes(void);
int sg_train_id_set(const int64_t *labels, int64_t n, int64_t ignore, int64_t *out, int cap, void *ws,
                    size_t ws_bytes, sg_stream_t stream);
/* The relabel itself: labels equal to sorted_ids[j] become mapped[j] (k ascending ids), in place. */
int sg_train_remap(int64_t *labels, int64_t n, const int64_t *sorted_ids, const int64_t *mapped, int k,
                   sg_stream_t stream);
/* getInstanceInfo (custom.py:76-90) for dense ids 0..k-1: pointnum, cls = semantic label of the first
 * point - cls_shift (-100 kept), pt_offset = float32(mean of xyz_middle) - xyz_middle in float64
 * (-100 - xyz_middle outside 0..k-1).  Sums are float64 in a fixed order: bitwise repeatable.
 * ws: sg_train_instance_workspace_bytes(n, k) bytes. */
size_t sg_train_instance_workspace_bytes(int64_t n, int k);
int sg_train_instance_info(const double *xyz_middle, const int64_t *inst, const int64_t *sem, int64_t n, int k,
                           int64_t cls_shift, int32_t *pointnum, int64_t *cls, double *pt_offset, void *ws,
                           size_t ws_bytes, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Test-time data transform (transform_test, custom.py:162-168, with getCroppedInstLabel and getInstanceInfo,
 * :170-194): sg_train_augment with the fixed rotation and no scale, sg_train_compact keeping every point,
 * sg_train_id_set / sg_train_remap and sg_train_instance_info, plus the entries below.
 * ---------------------------------------------------------------------------------------- */
/* S3DIS x4_split, pass 1 (s3dis.py:55-65): xyz_middle = xyz @ m in float64 (m_host as sg_train_augment's);
 * stats[3 b + a] = key of min(xyz_middle * scale) over piece b (points i with i % 4 == b) and axis a (keys as
 * above); stats[12] = 1 when some xyz_middle * scale is not finite, else 0. */
int sg_test_x4_minima(const float *xyz, int64_t n, const double *m_host, double scale, uint64_t *stats,
                      sg_stream_t stream);
/* S3DIS x4_split, pass 2 (s3dis.py:62-75): point i = 4 j + b goes to row (rows of pieces 0..b-1) + j:
 * coord = [b, trunc(xyz_middle * scale - min_host[3 b ..])] (int64 [n, 4], 16-byte aligned), xyz_middle,
 * feat (float32 [n, c]) and both labels. */
int sg_test_x4_split(const float *xyz, const float *feat, int c, const int64_t *sem, const int64_t *inst, int64_t n,
                     const double *m_host, double scale, const double *min_host, int64_t *coord,
                     double *xyz_middle, float *feat_out, int64_t *sem_out, int64_t *inst_out, sg_stream_t stream);
/* KITTIDataset.load's label decode (kitti.py:65-72): sem = lut[word & 0xFFFF] (the remapped learning map,
 * stuff 0..10, thing 11..18, ignore -100; INT32_MIN where the map has no key), inst = word where sem > 10,
 * else -100.  *missing = the smallest index whose key the map lacks, all ones when there is none (the caller
 * raises dict.__getitem__'s KeyError). */
int sg_kitti_decode_labels(const int32_t *words, int64_t n, const int32_t *lut, int64_t *sem, int64_t *inst,
                           uint64_t *missing, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Result files of the test loop (the reference's tools/test.py --out: save_single_instance :40-54,
 * save_gt_instance :68-77, save_panoptic_single :91-107) and their readers (tools/eval_det.py:29-32 reads the
 * masks back with split()).  The entries produce and parse the files' BYTES in device memory; the caller
 * moves them between pinned memory and the files.  Nothing synchronises unless stated.
 * ---------------------------------------------------------------------------------------- */
/* Mask text from runs: np.savetxt(path, rle_decode(rle), fmt='%d') (test.py:52-53) for masks first ..
 * first + count - 1 of n_inst masks over `length` points, whose runs are those of sg_instance_runs (int32
 * starts and exclusive ends, ascending and disjoint inside a mask; runs of mask k = [bounds[k], bounds[k+1])
 * of the n_runs runs).  text (16-byte aligned, text_capacity >= count * length * 2 bytes) receives, mask after
 * mask, '0' or '1' and '\n' per point: the file of mask first + j is text[j * length * 2 .. (j + 1) * length * 2). */
int sg_mask_text_runs(const int32_t *starts, const int32_t *ends, const int64_t *bounds, int64_t n_runs, int n_inst,
                      int64_t length, int first, int count, uint8_t *text, int64_t text_capacity, sg_stream_t stream);
/* The same bytes from bit rows uint32 [n_inst, ceil(length / 32)] (sg_instances_result.bits: point i of mask k
 * is bit i % 32 of word i / 32 of row k): the path of a caller that writes straight after the scan. */
int sg_mask_text_bits(const uint32_t *bits, int n_inst, int64_t length, int first, int count, uint8_t *text,
                      int64_t text_capacity, sg_stream_t stream);
/* Decimal lines: np.savetxt(path, values, fmt='%d') (test.py:77) for int64 values[n], exact over the whole
 * int64 range; n <= 102 261 125 (int32 text offsets).  With nyu_table (int32 [nyu_len], device) the values
 * first take save_gt_instance's remap (test.py:70-76, floor division): sem = v // 1000, ins = v % 1000,
 * v' = nyu_table[sem - 1] * 1000 + ins, and ins alone where sem == 0 (no table read); a negative sem - 1
 * indexes from the end like numpy.  meta (device int64 [3]): [0] = bytes of text, [1] = values whose table
 * index is outside the table (the reference's IndexError; their line is "0"), [2] = lines that did not fit
 * text_capacity (dropped; 21 bytes per value always fit).  ws: sg_decimal_lines_workspace_bytes(n). */
size_t sg_decimal_lines_workspace_bytes(int64_t n);
int sg_decimal_lines(const int64_t *values, int64_t n, const int32_t *nyu_table, int nyu_len, uint8_t *text,
                     int64_t text_capacity, int64_t *meta, void *ws, size_t ws_bytes, sg_stream_t stream);
/* save_panoptic_single (test.py:91-107): out[i] = (lut[words[i] & 0xFFFF] & 0xFFFF) | (words[i] & 0xFFFF0000).
 * lut int32 [lut_len <= 65536] is the reference's new_learning_map_inv (test.py:95-103) as a table, INT32_MIN
 * where it has no key; classes >= lut_len have none either.  `missing` (device uint64 [2]) is scratch.
 * SYNCHRONISES `stream`: missing_host[0] = points whose class has no entry, [1] = the first such point, [2] =
 * its class (all ones when there is none); returns SG_ERR_UNSUPPORTED when [0] != 0 (np.vectorize raises
 * KeyError there; out then holds the other points' words). */
int sg_panoptic_kitti_words(const uint32_t *words, int64_t n, const int32_t *lut, int lut_len, uint32_t *out,
                            uint64_t *missing, uint64_t *missing_host, sg_stream_t stream);
/* Readers.  Text of "%d\n" lines (optional '-', 1 to 19 digits, '\n'; the last '\n' may be missing) ->
 * values[line], at most `capacity` of them.  meta (device int64 [2]): [0] = lines, [1] = lines that are
 * anything else, outside int64 or beyond capacity (the caller then parses on the host).  nbytes < 2^31.
 * ws: sg_parse_decimal_lines_workspace_bytes(nbytes). */
size_t sg_parse_decimal_lines_workspace_bytes(int64_t nbytes);
int sg_parse_decimal_lines(const uint8_t *text, int64_t nbytes, int64_t *values, int64_t capacity, int64_t *meta,
                           void *ws, size_t ws_bytes, sg_stream_t stream);
/* Mask text ('0' | '1', '\n' per point; the last '\n' may be missing) of n = ceil(nbytes / 2) points ->
 * flags uint8 [n] (0 | 1; may be NULL; 16-byte aligned like text) and bits uint32 [ceil(n / 32)] (may be NULL;
 * stored a word at a time, so any uint32 address will do: a row of a [n_inst, ceil(n / 32)] table).
 * meta (device int64 [2]): [0] = n, [1] = points that are anything else. */
int sg_parse_mask_text(const uint8_t *text, int64_t nbytes, uint8_t *flags, uint32_t *bits, int64_t *meta,
                       sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Raw point-cloud text (csrc/cloud_io.hip, csrc/decimal.h): a delimited table of decimal numbers -> float64,
 * what the reference's preparations read with pandas.read_csv (dataset/s3dis/prepare_data_inst.py:65,84,
 * dataset/stpls3d/prepare_data_inst_instance_stpls3d.py:39,77) and the vertex lines of an ASCII PLY.
 * Numbers: [+-]? (D+ ('.' D*)? | '.' D+) ([eE] [+-]? D+)?, converted to the nearest double, ties to even -- what
 * Python's float() returns, bit for bit -- when the digits without leading zeros are at most 19 and the decimal
 * exponent of that integer lies in -27..27 (any zero with at most 4 exponent digits is a signed zero).  DECLINED,
 * never converted wrong: longer digit strings, exponents outside, [+-]? (inf | infinity | nan) in any case.
 * Malformed: every other token, and tokens above 64 bytes.
 *
 * Host entry over n tokens text[begin[k] .. begin[k] + len[k]): value[k] for status 0 (untouched otherwise),
 * status[k] = 0 ok | 1 declined | 2 malformed.  All pointers are host pointers. */
int sg_decimal_to_double_host(const uint8_t *text, const int64_t *begin, const int32_t *len, int64_t n, double *value,
                              uint8_t *status);
/* Lines end with '\n' (the last one may be missing; "\r\n" is accepted: '\r' is a blank like space and tab).  A
 * line of blanks alone, and with comment >= 0 a line whose first byte that is no blank equals `comment`, is no
 * row; the rows are the other lines behind the first skip_lines physical lines.  nbytes < 2^31 (scan values and
 * offsets are int32).  ws: sg_text_table_workspace_bytes(nbytes) for both calls.  Nothing synchronises.
 * meta (device int64 [8]), written by both calls: [0] physical lines, [1] rows, [2] byte offset where the data
 * begins (nbytes when there are not that many lines); sg_text_table_parse adds [3] rows with a declined field,
 * [4] malformed rows, [5] the lowest 1-based physical line of a malformed row (INT64_MAX: none), [6] 1 when [1]
 * differs from the `rows` passed. */
size_t sg_text_table_workspace_bytes(int64_t nbytes);
int sg_text_table_count(const uint8_t *text, int64_t nbytes, int64_t skip_lines, int comment, int64_t *meta, void *ws,
                        size_t ws_bytes, sg_stream_t stream);
/* values float64 [rows, cols] row-major, 1 <= cols <= 64; row_status uint8 [rows]: bit 0 = at least one field
 * declined (its value slot is left untouched, the row's other fields are valid), bit 1 = malformed (a field
 * count other than cols, a malformed token, an empty field under a character delimiter, a byte outside
 * printable ASCII, tab and '\r'; the row's value slots are undefined); row_line int32 [rows]: the 1-based
 * physical line of every row.  delimiter < 0: fields are separated by runs of blanks, blanks at either end of
 * a line are ignored.  delimiter = c (printable, no blank): exactly one c between two fields, blanks around a
 * field are ignored, a c in front of the line's end is an empty field.  With meta[6] set (the text holds more
 * or fewer rows than `rows`) the first min(rows, meta[1]) rows are written and nothing beyond the arrays. */
int sg_text_table_parse(const uint8_t *text, int64_t nbytes, int64_t skip_lines, int comment, int delimiter, int cols,
                        int64_t rows, double *values, uint8_t *row_status, int32_t *row_line, int64_t *meta, void *ws,
                        size_t ws_bytes, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Point-cloud pictures of a test run (the reference's tools/visualization.py: get_coords_color :141-231 and
 * write_ply :234-260), csrc/viz_io.hip.  Labels, colours and the PLY's vertex text are produced in device
 * memory; the caller reads the files, moves the text to pinned memory and writes it.  Nothing synchronises.
 * ---------------------------------------------------------------------------------------- */
/* The instance_pred paint (visualization.py:211-220: masks visited from the lowest score to the highest, each
 * overwriting `inst_label[mask == 1] = i`) without the order dependence: label[i] (int32 [n]) = the mask that
 * covers point i, is not skipped, and has the highest priority[k] (int32 [n_inst]; NULL = all equal; among equal
 * priorities the higher index), or -100 where there is none.  skip (uint8 [n_inst], may be NULL): the masks
 * below the confidence cut (:215-216).  pointnum[k] (int32 [n_inst]) = the whole population of mask k
 * (`ins_pointnum[i] = mask.sum()`, :219; not what the paint leaves of it), 0 for a skipped mask.  Masks as bit
 * rows uint32 [n_inst, ceil(n / 32)] (point i of mask k is bit i % 32 of word i / 32 of row k; bits at and beyond
 * n are ignored) ... */
int sg_viz_paint_bits(const uint32_t *bits, int n_inst, int64_t n, const int32_t *priority, const uint8_t *skip,
                      int32_t *label, int32_t *pointnum, sg_stream_t stream);
/* ... or as the runs of sg_mask_text_runs (int32 starts and exclusive ends, ascending and disjoint inside a mask,
 * runs of mask k = [bounds[k], bounds[k+1]) of the n_runs runs); ws: sg_viz_paint_runs_workspace_bytes(n_inst, n),
 * which holds the bit rows the runs are expanded to. */
size_t sg_viz_paint_runs_workspace_bytes(int n_inst, int64_t n);
int sg_viz_paint_runs(const int32_t *starts, const int32_t *ends, const int64_t *bounds, int64_t n_runs, int n_inst,
                      int64_t n, const int32_t *priority, const uint8_t *skip, int32_t *label, int32_t *pointnum,
                      void *ws, size_t ws_bytes, sg_stream_t stream);
/* The instance_gt labels (visualization.py:150-151 and :186-188): label[i] (int32 [n]) = ids[i] % 1000 - 1 with
 * numpy's floor modulo, i.e. -1 .. 998, and pointnum (int32 [999]) = the points of every label >= 0. */
int sg_viz_gt_labels(const int64_t *ids, int64_t n, int32_t *label, int32_t *pointnum, sg_stream_t stream);
/* The colour order of the instances (visualization.py:189 and :221, `np.argsort(ins_pointnum)[::-1]`, whose tie
 * order numpy leaves open) with the project's rule: rank[k] (int32 [n_inst]) = the position of instance k when the
 * instances are ordered by descending pointnum, the HIGHER index first among equal counts (a stable ascending
 * sort read backwards).  ws: sg_viz_instance_rank_workspace_bytes(n_inst). */
size_t sg_viz_instance_rank_workspace_bytes(int n_inst);
int sg_viz_instance_rank(const int32_t *pointnum, int n_inst, int32_t *rank, void *ws, size_t ws_bytes,
                         sg_stream_t stream);
/* rgb (uint8 [n, 3]) per point, as write_ply prints it (`int(c * 255)` of `rgb / 255`, :255-257 and :277):
 *   SG_VIZ_INPUT       from colors (float32 [n, 3]): ((c + 1) * 127.5) / 255 * 255 in float32, operation by
 *                      operation, truncated (:152, :277, :255)
 *   SG_VIZ_CLASS       table[cls[i]] for cls (int64 [n]) >= 0, zero below (semantic_gt, :155-158)
 *   SG_VIZ_CLASS_WRAP  table[cls[i]], a negative class indexing from the end like numpy (semantic_pred, :164-165)
 *   SG_VIZ_INSTANCE    table[rank[inst[i]] % k] for inst (int32 [n]) >= 0, zero below (:190-192, :222-224);
 *                      rank int32 [n_rank]
 * table: uint8 [k, 3].  meta (device int64 [3]): [0] = labels outside the table or the ranks (the reference's
 * IndexError), [1] = NaN colour components (`int(nan)` raises), [2] = colour components outside 0..255, which a
 * uint8 cannot hold (the caller's host path prints those). */
#define SG_VIZ_INPUT 0
#define SG_VIZ_CLASS 1
#define SG_VIZ_CLASS_WRAP 2
#define SG_VIZ_INSTANCE 3
int sg_viz_colors(int mode, const float *colors, const int64_t *cls, const int32_t *inst, const int32_t *rank,
                  int n_rank, const uint8_t *table, int k, int64_t n, uint8_t *rgb, int64_t *meta,
                  sg_stream_t stream);
/* write_ply's vertex lines (visualization.py:253-257) for the points with keep[i] != 0 (uint8 [n]; NULL = all;
 * the `label != -100` filter of :227-229): "%f %f %f %d %d %d\n" of xyz (float32 [n, 3]; with offset, float32
 * [n, 3], of xyz + offset in float32: `xyz += offset_coords`, :178) and rgb (uint8 [n, 3]), point after point.
 * The floats are what '{:f}'.format(np.float32(x)) prints: the exact binary value rounded half to even at six
 * decimals, "-0.000000" for -0.0 and for every negative value that rounds to zero.  meta (device int64 [4]):
 * [0] = bytes of text, [1] = lines written, [2] = kept rows DECLINED -- a coordinate that is not finite or whose
 * magnitude is 2^31 or more; they leave no line, and the caller formats the file on the host instead -- [3] =
 * lines that did not fit text_capacity (69 bytes per point always fit).  n <= 29 826 160 (int32 text offsets).
 * ws: sg_viz_ply_vertices_workspace_bytes(n). */
size_t sg_viz_ply_vertices_workspace_bytes(int64_t n);
int sg_viz_ply_vertices(const float *xyz, const float *offset, const uint8_t *rgb, const uint8_t *keep, int64_t n,
                        uint8_t *text, int64_t text_capacity, int64_t *meta, void *ws, size_t ws_bytes,
                        sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The loss block of forward_train (softgroup/model/softgroup.py:152-255) as fused kernels, csrc/losses.hip.
 * Everything is float32, contiguous, row-major; labels are int64.  Nothing synchronises and nothing is read
 * back: sums and losses are device scalars, upstream gradients come as device scalars (NULL = zero).  Sums are
 * taken in double in a fixed order (per-workgroup partials in `ws`, added by one workgroup of a second kernel;
 * no float atomics, no arrival counters): two calls on the same inputs give the same bits.
 * ws of the three *_fwd entries: sg_loss_reduce_workspace_bytes().  n, n_proposal or m = 0 is a valid call
 * that gives the empty sums.  Class counts above 64 return SG_ERR_UNSUPPORTED (the caller keeps the torch form).
 * ---------------------------------------------------------------------------------------- */
size_t sg_loss_reduce_workspace_bytes(void);
/* point_wise_loss (softgroup.py:152-170): F.cross_entropy(semantic_scores [n, c], semantic_labels [n], weight
 * [c] or NULL, ignore_index = ignore_label) and the L1 offset loss over the points with instance_labels !=
 * ignore_label (pt_offsets, pt_offset_labels [n, 3]).  out (float [6]): [0] = sum w_i nll_i, [1] = sum w_i,
 * [2] = sum |delta| over the 3 components of the instance points, [3] = n_pos, [4] = semantic_loss = [0] / [1]
 * (NaN when every label is ignored, like torch), [5] = offset_loss = [2] / max([3], 1) (0 without an instance
 * point, :164-165).  Max-subtracted log-sum-exp; 1 <= c <= 64.
 * A label that is not ignore_label and lies outside [0, c) is a device assert in torch; HERE THE ROW IS TREATED
 * AS IGNORED (no contribution, zero gradient), so the kernels never index outside a row. */
int sg_pointwise_loss_fwd(const float *semantic_scores, const int64_t *semantic_labels, const float *weight,
                          int64_t ignore_label, const float *pt_offsets, const float *pt_offset_labels,
                          const int64_t *instance_labels, int64_t n, int c, float *out, void *ws, size_t ws_bytes,
                          sg_stream_t stream);
/* Its backward (what autograd derives from softgroup.py:159-168).  sums = `out` of the forward; g_semantic,
 * g_offset: device scalars.  d_scores [n, c] = g_semantic / [1] * w_i * (softmax - onehot), zero rows for ignored
 * points; d_offsets [n, 3] = g_offset / max([3], 1) * sign(delta) on instance points (sign(0) = 0), zero elsewhere.
 * Either output may be NULL and is then skipped (a frozen backbone). */
int sg_pointwise_loss_bwd(const float *semantic_scores, const int64_t *semantic_labels, const float *weight,
                          int64_t ignore_label, const float *pt_offsets, const float *pt_offset_labels,
                          const int64_t *instance_labels, int64_t n, int c, const float *sums,
                          const float *g_semantic, const float *g_offset, float *d_scores, float *d_offsets,
                          sg_stream_t stream);
/* Proposal -> class label (softgroup.py:194-222).  ious_on_cluster [n_proposal, n_gt] (finite), instance_cls
 * [n_gt]; GTs with instance_cls == ignore_label are background and count as IoU -1 (the reference drops their
 * columns, :195-197).  A proposal whose largest IoU reaches pos_iou_thr takes that GT (lowest column among equal
 * IoUs, torch's max); with match_low_quality every GT whose column maximum reaches min_pos_thr also claims its
 * best proposal (lowest row among equals), and where several GTs claim one proposal the highest GT index wins
 * (the loop of :215-217, later overwrites earlier).  labels [n_proposal] = instance_cls of the assigned GT, or
 * background_label.  n_gt >= 1.  ws (only with match_low_quality): sg_assign_proposals_workspace_bytes. */
size_t sg_assign_proposals_workspace_bytes(int n_proposal);
int sg_assign_proposals(const float *ious_on_cluster, const int64_t *instance_cls, int64_t ignore_label,
                        float pos_iou_thr, int match_low_quality, float min_pos_thr, int64_t background_label,
                        int n_proposal, int n_gt, int64_t *labels, void *ws, size_t ws_bytes, sg_stream_t stream);
/* cls_loss and iou_score_loss (softgroup.py:223-224, 240-255).  cls_scores, iou_scores [n_proposal, k1] with
 * k1 = K + 1 classes (2 <= k1 <= 64, class K = background); ious_on_pred [n_proposal, n_gt] as
 * sg_get_mask_iou_on_pred returns it.  gt_iou [n_proposal] (output, kept for the backward) = row maximum over the
 * foreground GTs.  out (float [6]): [0] = sum of the rows' cross entropy, [1] = sum w (iou_scores[p, label] -
 * gt_iou)^2 with w = [label < K], [2] = num_pos = sum w, [3] = num_neg, [4] = cls_loss = [0] / n_proposal,
 * [5] = iou_score_loss = [1] / ([2] + 1).  Rows whose label lies outside [0, K] contribute nothing. */
int sg_proposal_loss_fwd(const float *cls_scores, const float *iou_scores, const int64_t *labels,
                         const float *ious_on_pred, const int64_t *instance_cls, int64_t ignore_label,
                         int n_proposal, int n_gt, int k1, float *gt_iou, float *out, void *ws, size_t ws_bytes,
                         sg_stream_t stream);
/* d_cls_scores = g_cls / n_proposal * (softmax - onehot); d_iou_scores = g_iou / ([2] + 1) * 2 w (s - gt_iou) in
 * the label's column, zero in the others (whole rows are written).  Either output may be NULL. */
int sg_proposal_loss_bwd(const float *cls_scores, const float *iou_scores, const int64_t *labels,
                         const float *gt_iou, const float *sums, const float *g_cls, const float *g_iou,
                         int n_proposal, int k1, float *d_cls_scores, float *d_iou_scores, sg_stream_t stream);
/* mask_loss (softgroup.py:226-238) over the m proposal points.  mask_scores [m, k1], instance_batch_idxs int32
 * [m] (the proposal of every point), labels [n_proposal], mask_label [m] as sg_get_mask_label returns it (-1 =
 * ignored).  mask_sig [m] = sigmoid(mask_scores[i, labels[instance_batch_idxs[i]]]), what sg_get_mask_iou_on_pred
 * consumes.  out (float [6]): [0] = sum of F.binary_cross_entropy's terms -(y max(log p, -100) + (1 - y)
 * max(log(1 - p), -100)) over the points with y != -1, [1] = their number, [4] = mask_loss = [0] / ([1] + 1).
 * p, the logarithms and the gradient are evaluated in double from the float logit: where a float sigmoid already
 * rounds to 1 (logits of 17 to 36) the result is the float64 one, not the clamp.  A point whose proposal or class
 * index is out of range is ignored (mask_sig 0). */
int sg_mask_loss_fwd(const float *mask_scores, const int32_t *instance_batch_idxs, const int64_t *labels,
                     const float *mask_label, int64_t m, int n_proposal, int k1, float *mask_sig, float *out,
                     void *ws, size_t ws_bytes, sg_stream_t stream);
/* d_mask_scores [m, k1]: g_mask * w (p - y) / max(p (1 - p), 1e-12) * p (1 - p) / ([1] + 1) in the class column
 * (binary_cross_entropy's backward followed by the sigmoid's, including the zero at saturated logits), zero in
 * the other columns; every element is written. */
int sg_mask_loss_bwd(const float *mask_scores, const int32_t *instance_batch_idxs, const int64_t *labels,
                     const float *mask_label, const float *sums, const float *g_mask, int64_t m, int n_proposal,
                     int k1, float *d_mask_scores, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The optimizer step as multi-tensor kernels, csrc/optim.hip: gradient norm and clip coefficient
 * (torch.nn.utils.clip_grad_norm_), AMP unscale / skip (torch.amp.GradScaler) and the Adam / AdamW / SGD update of
 * torch.optim.  Parameters, gradients and states are float32 and contiguous.  Nothing synchronises and nothing is
 * read back.
 *
 * table: device int64 [SG_OPTIM_TABLE_ROWS, n_tensors], one column per tensor: the device addresses of the
 * parameter, its gradient, its two states (exp_avg, exp_avg_sq / momentum_buffer, unused) and its step counter
 * (a float32 scalar, as torch keeps it with capturable=True), and the element count.  Tensors need no alignment
 * beyond their 4 bytes (views at an odd element offset are fine: 16-byte accesses are used where all arrays of a
 * tensor share their address modulo 16, scalar ones elsewhere).  chunks: device int64 [n_chunks, 3] = (tensor,
 * first element, elements), as sg_optim_plan writes it.  There is no limit on n_tensors.  n_chunks = 0 (no
 * tensor, or only empty ones) is a valid call that launches nothing.
 * grad_scale, found_inf: GradScaler's device scalars or NULL (scale 1, never skipped): the gradient counts as
 * g / grad_scale, and with *found_inf != 0 a step entry writes nothing at all -- no parameter, no state, no counter.
 * clip_coef: device scalar or NULL (1), out + 1 of sg_optim_grad_norm.
 * Every element is updated in double from its float32 inputs and each stored value rounded once.
 * ---------------------------------------------------------------------------------------- */
#define SG_OPTIM_ROW_PARAM 0
#define SG_OPTIM_ROW_GRAD 1
#define SG_OPTIM_ROW_STATE0 2
#define SG_OPTIM_ROW_STATE1 3
#define SG_OPTIM_ROW_STEP 4
#define SG_OPTIM_ROW_COUNT 5
#define SG_OPTIM_TABLE_ROWS 6
/* elements per chunk (fixed) */
int sg_optim_chunk_elems(void);
/* HOST code.  The chunk table of tensors with counts[t] elements (host int64 [n_tensors]): tensor after tensor,
 * every element in exactly one chunk, no chunk across two tensors, none longer than sg_optim_chunk_elems(); an
 * empty tensor has no chunk.  Returns the number of chunks (>= 0) and writes them to chunks (host int64
 * [chunk_capacity, 3]); chunk_capacity = 0 only counts.  Negative: SG_ERR_ARG (a negative count, a null array), or
 * SG_ERR_WORKSPACE when chunk_capacity is not 0 and too small. */
int64_t sg_optim_plan(const int64_t *counts, int n_tensors, int64_t *chunks, int64_t chunk_capacity);
/* bytes of ws for sg_optim_grad_norm (the per-workgroup partial sums) */
size_t sg_optim_workspace_bytes(void);
/* Two launches: the L2 norm over all gradients (as g / grad_scale), summed in double in a fixed order (per-workgroup
 * partials in ws, added by one workgroup; no float atomics, no arrival counters: two calls give the same bits).
 * out (device float [4]): [0] = norm, [1] = clip_coef = min(1, max_norm / (norm + 1e-6)) in float32, the formula of
 * clip_grad_norm_ (NaN stays NaN), [2] = 1 if any g / grad_scale is not finite, else 0, [3] = 0.  With n_chunks = 0
 * nothing is launched and out keeps what it holds. */
int sg_optim_grad_norm(const int64_t *table, int n_tensors, const int64_t *chunks, int64_t n_chunks,
                       const float *grad_scale, float max_norm, float *out, void *ws, size_t ws_bytes,
                       sg_stream_t stream);
/* One launch: torch.optim.Adam (adamw = 0: g += weight_decay * p) or AdamW (adamw = 1: p *= 1 - lr * weight_decay)
 * with g = grad / grad_scale * clip_coef, step = counter + 1:
 *   m = m + (1 - beta1) (g - m);  v = beta2 v + (1 - beta2) g g;
 *   p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * and advances every tensor's counter.  zero_grad != 0 writes zeros to the gradient after reading it.
 * arrive: device int32 [n_tensors], zero before the first call; every call that returns SG_OK leaves it zero
 * (the chunks of a tensor count themselves there, the last one advances the step counter). */
int sg_optim_adam_step(const int64_t *table, int n_tensors, const int64_t *chunks, int64_t n_chunks, double lr,
                       double beta1, double beta2, double eps, double weight_decay, int adamw,
                       const float *grad_scale, const float *found_inf, const float *clip_coef, int zero_grad,
                       int32_t *arrive, sg_stream_t stream);
/* One launch: torch.optim.SGD.  g += weight_decay * p;  with momentum != 0: buf = g where the counter is 0 (torch's
 * first step), else buf = momentum buf + (1 - dampening) g;  g = nesterov ? g + momentum buf : buf;  p -= lr g.
 * buf is STATE0 (unused and may be 0 with momentum = 0).  The counter advances like Adam's. */
int sg_optim_sgd_step(const int64_t *table, int n_tensors, const int64_t *chunks, int64_t n_chunks, double lr,
                      double momentum, double dampening, double weight_decay, int nesterov, const float *grad_scale,
                      const float *found_inf, const float *clip_coef, int zero_grad, int32_t *arrive,
                      sg_stream_t stream);
/* One launch: g *= *coef in float32 for every gradient of the table (the second half of clip_grad_norm_). */
int sg_optim_scale_grads(const int64_t *table, int n_tensors, const int64_t *chunks, int64_t n_chunks,
                         const float *coef, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Thinning a cloud and carrying results back to every original point (csrc/resample.hip).  The reference has NO
 * counterpart on the device: dataset/s3dis/downsample.py draws a random sample on the host and raises for
 * --voxel-size; nothing there re-expresses a result over the full cloud.  All of it is opt-in.  Arithmetic is
 * integer and IEEE double, selection uses integer atomics only: two calls on the same input give the same bytes.
 * Every probe loop is bounded by the table capacity (a power of two >= 2 n), every shell walk by a fixed shell
 * count, and every index read from memory is range-checked before it is used as an address.
 *
 * VOXEL-GRID DOWNSAMPLE.  xyz float32 [n, 3] (device), 0 <= n < 2^31, voxel a finite double > 0.
 * Cell of a point, per axis: c = floor((double)x / voxel) -- one IEEE double division, not a product with the
 * reciprocal.  A point is INVALID when a coordinate is not finite or |c| >= 2^31: any invalid point sets bit 0 of
 * meta[1], and then no table is touched, meta[0] = 0 and inverse is all -1 (the flag is decided by a kernel of its
 * own, before the kernel that inserts).  Representative of an occupied voxel: SG_PICK_FIRST the lowest point index
 * in it; SG_PICK_CENTER the point with the smallest d2 = (dx*dx + dy*dy) + dz*dz, dx = (double)x - ((double)c + 0.5)
 * * voxel (double, in that order), the lowest index among equal d2.
 * sample_ids int32 [>= n]: the representatives in ASCENDING index order (the thinned cloud keeps the point order),
 * the first meta[0] entries written; inverse int32 [n]: position in sample_ids of the representative of point i's
 * voxel; meta int32 [2]: [0] = occupied voxels, [1] = flags.  n = 0 writes meta = {0, 0}. */
#define SG_PICK_FIRST 0
#define SG_PICK_CENTER 1
size_t sg_grid_downsample_workspace_bytes(int n);
int sg_grid_downsample(const float *xyz, int n, double voxel, int pick, int32_t *sample_ids, int32_t *inverse,
                       int32_t *meta, void *ws, size_t ws_bytes, sg_stream_t stream);
/* EXACT NEAREST SOURCE POINT.  src float32 [n_src, 3], query float32 [n_query, 3], 1 <= n_src < 2^31,
 * 0 <= n_query < 2^31.  index[q] = the source j with the smallest d2 = (dx*dx + dy*dy) + dz*dz, dx = (double)qx -
 * (double)sx (double, in that order), the LOWEST j among equal d2.  With max_dist >= 0 a query whose smallest d2
 * exceeds max_dist * max_dist gets -1 (max_dist < 0: no limit).  dist2 (double [n_query], may be NULL) = that d2,
 * +inf where index is -1.  The result equals the brute force over all sources for every query and every cell > 0.
 *
 * The grid is a means: sources are counted into a hashed uniform grid of `cell` (cell index floor((double)x / cell),
 * |index| < 2^30, else the grid is not used at all), a query walks the shells of cells at Chebyshev distance 0, 1, 2
 * around its own cell and stops after shell R once its best d2 < (R cell)^2 (1 - 2^-18) (after shell 0: once it is
 * exactly 0) -- the margin covers the rounding of the cell assignment, which moves a cell face by at most 2^-22
 * cells.  A query not decided after shell 2 (far from every source, in a gap between clusters, outside the grid's
 * range) goes onto a device work list and a second kernel answers it by a scan of ALL sources, one workgroup per
 * query, with the same (d2, j) order: such a query costs one scan, never an unbounded walk.
 * sg_nearest_default_cell (host): about two sources per cell -- with e_k = hi_k - lo_k the extents of the source
 * bounding box that are > 0 and d their number, cell = (2 * prod e_k / n_src)^(1/d) (1 when d = 0), and at least
 * max|coordinate| / 2^29 so that the whole box stays inside the grid's range.
 * meta int32 [2], shared by the two calls: sg_nearest_build zeroes it and sets flag bit 0 of meta[1] for a source
 * coordinate that is not finite (bit 2: the grid is out of range and unused -- not an error); sg_nearest_query sets
 * bit 1 for such a query coordinate (its index is -1) and leaves in meta[0] the number of queries the full scan
 * answered.  With bit 0 set every index is -1 and nothing is scanned: the error costs O(n_query).  grid: >= sg_nearest_grid_bytes(n_src) bytes that sg_nearest_build fills and any number of queries with
 * the same src, n_src and cell read. */
double sg_nearest_default_cell(const double *lo, const double *hi, int64_t n_src);
size_t sg_nearest_grid_bytes(int n_src);
int sg_nearest_build(const float *src, int n_src, double cell, void *grid, size_t grid_bytes, int32_t *meta,
                     sg_stream_t stream);
size_t sg_nearest_query_workspace_bytes(int n_query);
int sg_nearest_query(const float *src, int n_src, double cell, const void *grid, size_t grid_bytes, const float *query,
                     int n_query, double max_dist, int32_t *index, double *dist2, int32_t *meta, void *ws,
                     size_t ws_bytes, sg_stream_t stream);
/* MASKS THROUGH AN INDEX MAP.  bits uint32 [n_inst, ceil(n_src / 32)] (the bit rows of sg_mask_nms), index int32
 * [n_out] -> out uint32 [n_inst, ceil(n_out / 32)]: bit i of row k = bit index[i] of source row k, 0 where
 * index[i] < 0; bits at and beyond n_out are written as 0 and every word of every row is written.  An index >=
 * n_src is a caller error that reads nothing: it counts as -1 and sets bit 0 of *meta (int32, may be NULL; zeroed
 * by the call). */
int sg_mask_bits_gather(const uint32_t *bits, int n_inst, int64_t n_src, const int32_t *index, int64_t n_out,
                        uint32_t *out, int32_t *meta, sg_stream_t stream);
/* Bit rows -> runs, in two passes over the same workspace (>= sg_mask_runs_workspace_bytes; 0 = outside the range
 * n_points < 2^31 and n_inst * ceil(n_points / 2) < 2^31, the calls then return SG_ERR_UNSUPPORTED).  The count pass
 * writes bounds int64 [n_inst + 1], the exclusive prefix of the runs per row with the total in bounds[n_inst]; the
 * fill pass writes the first `capacity` runs: starts / ends int32, 0-based, end exclusive, ascending, maximal --
 * what sg_rle_format_device and sg_mask_bits_from_runs take.  Bits at and beyond n_points are ignored. */
size_t sg_mask_runs_workspace_bytes(int n_inst, int64_t n_points);
int sg_mask_runs_count(const uint32_t *bits, int n_inst, int64_t n_points, int64_t *bounds, void *ws, size_t ws_bytes,
                       sg_stream_t stream);
int sg_mask_runs_fill(const uint32_t *bits, int n_inst, int64_t n_points, const void *ws, size_t ws_bytes,
                      int32_t *starts, int32_t *ends, int64_t capacity, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Large clouds: overlapping tiles, one scan per tile at full resolution, instances that straddle a cut joined
 * again (csrc/stitch.hip).  The reference only cuts blocks offline (dataset/stpls3d/
 * prepare_data_inst_instance_stpls3d.py) and evaluates every block as a scene of its own.  All of it is opt-in.
 * Arithmetic is integer and IEEE double, selection uses integer atomics only (compare-and-swap on a key, OR on
 * bits), orders come from the stable radix sort: two calls on the same input give the same bytes.  Every probe loop
 * is bounded by the table capacity, every binary search by 32 steps, the component rounds by the instance count;
 * every index read from memory is range-checked before it is used as an address; no workgroup waits for another.
 *
 * TILES.  xyz float32 [n, 3] (device), 0 <= n < 2^29 on the device (the numpy twin: n < 2^31), size a finite double
 * > 0, 0 <= margin <= size / 2, origin (ox, oy) finite doubles.  Tiles split x and y only.
 * Core cell of a point, per axis: c = floor(((double)x - o) / size) -- one subtraction, one division.  A point is
 * INVALID when a coordinate (z included) is not finite or |c| >= 2^30: any invalid point sets bit 0 of meta[1], and
 * then no table is touched and meta[0] = meta[2] = 0 (the flag is decided by a kernel of its own, before the kernel
 * that inserts).  The tiles are the cells that hold at least one core point, numbered in ascending (cy, cx) order;
 * more than 65535 of them set bit 1 of meta[1].
 * Overlap: with margin == 0 a point belongs to its core tile only.  Otherwise, per axis, lo = o + (double)c * size,
 * hi = o + (double)(c + 1) * size; the point also belongs on the side c - 1 when (double)x < lo + margin, else on
 * the side c + 1 when (double)x >= hi - margin (each expression in that order, in double; the "else" only matters
 * where rounding at margin == size / 2 makes both hold).  The two axes combine: core, x side, y side and the
 * diagonal, so a point has 1, 2 or 4 candidate cells -- and it joins a neighbouring cell only if that cell is a tile
 * (fewer tiles, 3 among them, only next to a hole of the tile grid).
 * The count pass writes meta int32 [4]: [0] = T tiles, [1] = flags, [2] = total = entries of tile_points, and keeps
 * its state in ws (>= sg_tile_assign_workspace_bytes(n); 0 = n outside the range).  After one read-back of meta the
 * fill pass (same xyz, n, size, margin, origin and ws; ws2 >= sg_tile_assign_fill_workspace_bytes(total)) writes
 * tile_cells int32 [T, 2] = (cx, cy), tile_off int64 [T + 1], tile_points int32 [total]: the ASCENDING point indices
 * of tile t at tile_off[t] .. tile_off[t+1] (a tile keeps the cloud's point order; the order comes from a stable
 * sort of (tile, point) pairs generated in point order), core_tile int32 [n] and core_pos int32 [n]: the position
 * of point i in its core tile's list.  The fill pass must not be called when meta[1] != 0. */
size_t sg_tile_assign_workspace_bytes(int n);
size_t sg_tile_assign_fill_workspace_bytes(int64_t total);
int sg_tile_assign_count(const float *xyz, int n, double size, double margin, double ox, double oy, int32_t *meta,
                         void *ws, size_t ws_bytes, sg_stream_t stream);
int sg_tile_assign_fill(const float *xyz, int n, double size, double margin, double ox, double oy, int n_tiles,
                        int64_t total, int32_t *tile_cells, int64_t *tile_off, int32_t *tile_points,
                        int32_t *core_tile, int32_t *core_pos, const void *ws, size_t ws_bytes, void *ws2,
                        size_t ws2_bytes, sg_stream_t stream);
/* SHARED POINTS of two strictly ascending int32 lists a [n_a], b [n_b]: pos_a / pos_b int32 [>= min(n_a, n_b)] = the
 * positions in each list of the common elements, ascending, the first *count (device int32) entries written.  A
 * binary search per element of a and an ordered compaction (a prefix sum).  ws >= sg_tile_shared_workspace_bytes. */
size_t sg_tile_shared_workspace_bytes(int n_a);
int sg_tile_shared(const int32_t *a, int n_a, const int32_t *b, int n_b, int32_t *pos_a, int32_t *pos_b,
                   int32_t *count, void *ws, size_t ws_bytes, sg_stream_t stream);
/* LINKS between the instances of two tiles.  bits_a uint32 [n_a, W], bits_b uint32 [n_b, W], W = ceil(n_bits / 32):
 * the two tiles' masks restricted to the points S both tiles hold (sg_mask_bits_gather with the shared positions as
 * the index); bits at and beyond n_bits are ignored on both sides.  ca = population of row i of a = |M(g) n S|,
 * cb likewise, inter = popcount(a_i & b_j) = |M(g) n M(h)|; den = ca + cb - inter for SG_NMS_IOU, min(ca, cb) for
 * SG_NMS_MIN.  The pair is LINKED when labels_a[i] == labels_b[j], inter >= min_shared, den > 0 and
 * (double)inter / (double)den > thr, strictly -- one IEEE division, the rule of sg_mask_nms.  A link sets bit
 * base_b + j of row base_a + i and bit base_a + i of row base_b + j of adj uint32 [n_total, ceil(n_total / 32)]
 * (integer OR; the caller zeroes adj once).  adj may be NULL (no decision, labels unused).  Optional outputs:
 * inter_out int32 [n_a, n_b], cnt_a_out int32 [n_a], cnt_b_out int32 [n_b].
 * RANGE: n_total <= 16384, n_bits < 2^31, else SG_ERR_UNSUPPORTED. */
int sg_mask_cross_links(const uint32_t *bits_a, int n_a, const uint32_t *bits_b, int n_b, int64_t n_bits,
                        const int32_t *labels_a, const int32_t *labels_b, int base_a, int base_b, int n_total,
                        double thr, int measure, int min_shared, uint32_t *adj, int32_t *inter_out,
                        int32_t *cnt_a_out, int32_t *cnt_b_out, sg_stream_t stream);
/* OBJECTS: comp int32 [n_total], comp[g] = the smallest member of g's connected component in the symmetric
 * adjacency bit matrix (bits at and beyond n_total ignored).  One workgroup, labels in LDS, min-label propagation
 * with pointer jumping, at most n_total + 1 rounds.  n_total <= 16384, else SG_ERR_UNSUPPORTED. */
int sg_stitch_components(const uint32_t *adj, int n_total, int32_t *comp, sg_stream_t stream);
/* SET BITS AS GLOBAL IDS.  bits uint32 [n_inst, ceil(n_bits / 32)] (a tile's rows).  The count pass writes
 * cnt[k] = population of row k and core_cnt[k] = its set bits p with core[p] != 0 (core uint8 [n_bits], NULL = 0).
 * The fill pass writes for row k, in bit order from row_off[k] (int64, device): ids = map[p] (map int32 [n_bits],
 * the tile's point list) and keys = row_key[k] (int32; negative = no object, written as 0xFFFF).  A map value
 * outside [0, n_points) sets bit 0 of *meta (int32, zeroed by the caller) and the entry becomes (0, 0xFFFF).
 * Entries at and beyond `capacity` are not written. */
int sg_mask_bits_ids_count(const uint32_t *bits, int n_inst, int64_t n_bits, const uint8_t *core, int32_t *cnt,
                           int32_t *core_cnt, sg_stream_t stream);
int sg_mask_bits_ids_fill(const uint32_t *bits, int n_inst, int64_t n_bits, const int32_t *map, int64_t n_points,
                          const int64_t *row_off, const int32_t *row_key, int32_t *ids, uint32_t *keys,
                          int64_t capacity, int32_t *meta, sg_stream_t stream);
/* UNION of the members' ids per object as maximal runs -- no row over the full cloud exists anywhere: memory is
 * proportional to total = the sum of the mask populations.  ids int32 [total], keys uint32 [total] (object number;
 * an entry with key >= n_obj or id outside [0, n_points) belongs to no object).  The pairs are ordered by
 * (object, id) with two stable radix sorts; equal neighbours inside an object collapse, ids that differ by 1
 * continue a run.  The count pass writes bounds int64 [n_obj + 1] (exclusive prefix of the runs per object, the
 * total in bounds[n_obj]) and keeps the sorted pairs in ws; the fill pass writes the first `capacity` runs: starts /
 * ends int32, 0-based, end exclusive, ascending -- what sg_rle_format_device takes.
 * RANGE: n_obj <= 16384, total < 2^31, n_points < 2^31; beyond it sg_stitch_union_workspace_bytes returns 0 and
 * the calls SG_ERR_UNSUPPORTED -- nothing is truncated. */
size_t sg_stitch_union_workspace_bytes(int64_t total, int n_obj, int64_t n_points);
int sg_stitch_union_count(const int32_t *ids, const uint32_t *keys, int64_t total, int n_obj, int64_t n_points,
                          int64_t *bounds, void *ws, size_t ws_bytes, sg_stream_t stream);
int sg_stitch_union_fill(int64_t total, int n_obj, int64_t n_points, const void *ws, size_t ws_bytes, int32_t *starts,
                         int32_t *ends, int64_t capacity, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Several results over ONE cloud combined into one (csrc/ensemble.hip): the passes of test-time augmentation, the
 * folds of several checkpoints, a tiled next to a thinned result.  K passes (1 <= K <= 32) over the same n points in
 * the same order; pass p has an integer weight 1 <= w_p, W = sum w_p <= 32767.  The reference has no counterpart.
 * All of it is opt-in.  softgroup_amd.ops.ensemble's numpy twins are the definition and the device results equal
 * them byte for byte.  Arithmetic is integer apart from the one IEEE double division of the link rule; atomics are
 * integer only (OR on adjacency bits, ADD on populations): two calls on the same input give the same bytes.  Every
 * loop is bounded by an argument, every index read from memory is range-checked before it addresses anything, no
 * workgroup waits for another.
 *
 * LABEL VOTE.  labels int64 [K, n] (device, row p = pass p), weights int32 [K] (device), out int64 [n] (must not
 * overlap labels).  At point x the label of pass p is COUNTED when it is >= 0 and != ignore_label; count(c) = the
 * sum of w_p over the passes that say c.  out[x] = the class with the greatest count, the LOWEST class among equal
 * counts; a point with no counted label keeps labels[0, x].  There is no class cap: the winner is one of the at
 * most K distinct values, found by comparing the K labels of the point with each other in registers.  The weights
 * are the caller's to keep inside 1 .. 32767 with W <= 32767 (sums are int32; a weight outside the range changes
 * counts, it is never an address).  RANGE: 1 <= k <= 32, 0 <= n < 2^31, else SG_ERR_UNSUPPORTED. */
int sg_label_vote(const int64_t *labels /* [K, n] */, int k, int64_t n, const int32_t *weights /* device [K] */,
                  int64_t ignore_label, int64_t *out, sg_stream_t stream);
/* GROUP LINKS over one stacked mask matrix.  bits uint32 [n_total, W], W = ceil(n_bits / 32): the instances of all
 * passes, numbered g = 0 .. n_total-1 by (pass, list order); labels int32 [n_total]; group int32 [n_total] = the
 * pass of the row.  Bits at and beyond n_bits are ignored.  Rows g < h are LINKED when group[g] != group[h],
 * labels[g] == labels[h] and the rule of sg_mask_cross_links holds with ca, cb = the populations of the two rows and
 * inter = popcount(row g & row h), all over the n_bits points: inter >= min_shared, den > 0 and
 * (double)inter / (double)den > thr, strictly, den = ca + cb - inter for SG_NMS_IOU, min(ca, cb) for SG_NMS_MIN.
 * It is the kernel of sg_mask_cross_links on the matrix against itself, with the group test beside the label test
 * and the tile pairs below the diagonal skipped: ONE launch for all K (K - 1) / 2 pairs of passes.  A link sets bit h
 * of row g and bit g of row h of adj uint32 [n_total, ceil(n_total / 32)] (integer OR; the caller zeroes adj) --
 * what sg_stitch_components takes.  RANGE: n_total <= 16384, n_bits < 2^31, else SG_ERR_UNSUPPORTED. */
int sg_mask_group_links(const uint32_t *bits, int n_total, int64_t n_bits, const int32_t *labels, const int32_t *group,
                        double thr, int measure, int min_shared, uint32_t *adj, sg_stream_t stream);
/* MASK VOTE.  The objects are the connected components of the links.  obj_off int32 [n_obj + 1]: object o owns the
 * entries obj_off[o] .. obj_off[o+1] - 1 of members / member_weight / member_pass, int32 arrays of n_total entries
 * each (an instance belongs to at most one object) sorted by (object, pass): members[m] = the row g of bits,
 * member_pass[m] = its pass p, member_weight[m] = w_p.  For object o and point x, v = the sum of w_p over the passes
 * p that have at least one member of o containing x -- a pass counts ONCE per point, however many of its members
 * hold the point: the entries of one pass are adjacent, their words are OR-ed and the weight of the first of them is
 * added once.  Bit x of row o of out_bits uint32 [n_obj, W] is set when v >= need[o] (int32 [n_obj], 1 <= need);
 * npoint int32 [n_obj] = the population of the row.  Bits at and beyond n_bits are ignored in bits and 0 in
 * out_bits.  A lane owns one output word, the counts of its 32 points are 15 bit planes (v <= 32767) added by
 * ripple carry and compared with need from the top plane; one integer atomic per wave into npoint, which the call
 * zeroes first.
 * Nothing read from memory addresses anything unchecked: obj_off[o] and obj_off[o+1] are clamped into
 * [0, n_total] and to ascending order; an entry with members[m] outside [0, n_total), member_pass[m] outside
 * [0, 32) or member_weight[m] outside [1, 32767] is IGNORED (as if it were not in the list); an object whose
 * need is outside [1, 32767] gets an empty row; a sum beyond 32767 (only with weights the rules above exclude)
 * counts as reaching every need.  No error status is raised for any of them.
 * RANGE: n_total <= 16384, n_obj <= 16384, n_bits < 2^31, else SG_ERR_UNSUPPORTED -- nothing is truncated. */
int sg_mask_vote(const uint32_t *bits, int n_total, int64_t n_bits, const int32_t *obj_off /* [n_obj + 1] */,
                 const int32_t *members /* sorted by (object, pass) */, const int32_t *member_weight,
                 const int32_t *member_pass, const int32_t *need, int n_obj, uint32_t *out_bits, int32_t *npoint,
                 sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Superpoints for clouds that ship none (csrc/geometry.hip): the exact k nearest neighbours, normal and curvature
 * per point, and the connected components of "same smooth surface" links, whose ids sg_superpoint_index accepts as
 * they are.  The reference has no counterpart.  All of it is opt-in: nothing calls it unless asked.
 * softgroup_amd.ops.geometry's numpy twins are the definition; sg_knn and sg_grow_segments equal them byte for byte,
 * sg_point_normals to within the rounding of its eigen-solver.  Arithmetic is integer and IEEE double, selection by
 * comparisons and integer atomics only: two calls on the same input give the same bytes.  Every index read from
 * memory is range-checked before it addresses anything; every loop has a bound that does not depend on the data.
 *
 * K NEAREST OTHER POINTS.  xyz float32 [n, 3], 0 <= n < 2^31, 1 <= k <= SG_KNN_MAX_K (else SG_ERR_UNSUPPORTED and
 * sg_knn_workspace_bytes returns 0; nothing is launched).  d2 of two points = (dx*dx + dy*dy) + dz*dz, dx =
 * (double)x_i - (double)x_j (double, in that order).  Row i of idx int32 [n, k] / d2 double [n, k]: the k points
 * j != i with the smallest (d2, j) in lexicographic order, in that order -- a point with equal coordinates is a
 * neighbour at distance 0, ties at the k-th place go to the lower index.  With max_dist >= 0 a point with d2 >
 * max_dist * max_dist is no neighbour (max_dist < 0: no limit).  Missing entries (n - 1 < k, or beyond max_dist) are
 * -1 / +inf.  The result equals the brute force for every cell > 0.
 * SG_KNN_MAX_K is 32: a thread keeps its list in LDS, 12 bytes per entry, and 128 threads x 32 entries = 48 KB is
 * what stays below the 64 KB a kernel gets by default with three workgroups to a CU; 64 would leave one.
 * The grid is the one of sg_nearest_build (cell index floor((double)x / cell), |index| < 2^30).  A coordinate that is
 * not finite sets SG_KNN_FLAG_NOT_FINITE in meta[1], a cell index at or beyond 2^30 SG_KNN_FLAG_CELL_RANGE -- by a
 * kernel of its own, before any table is touched -- and then NO output row is written at all.  A query walks the
 * shells of cells at Chebyshev distance 0 .. SG_KNN_MAX_SHELL around its own cell and stops after shell R once it
 * holds k candidates and the k-th d2 < (R cell)^2 (1 - 2^-18) (after shell 0: once it is exactly 0).  With
 * max_dist >= 0 and ceil(max_dist / cell * (1 + 2^-20)) <= SG_KNN_MAX_SHELL the walk ends after that many shells
 * and decides every query.  A query not decided by the walk goes onto a device work list and is answered by a scan
 * of ALL points, one wave per query, with the same (d2, j) order: it costs one scan, never an unbounded walk.
 * meta int32 [4]: [0] = queries the full scan answered, [1] = flags, [2], [3] = 0.  n = 0 writes meta only.
 * sg_knn_default_cell (host): about k / 2 points per cell were the cloud spread evenly over its bounding box --
 * with e_d = hi_d - lo_d the extents that are > 0 and D their number, cell = (max(k, 2) / 2 * prod e_d / n)^(1/D)
 * (1 when D = 0), and at least max|coordinate| / 2^29 so that the whole box stays inside the grid's range.  Scanned
 * clouds are surfaces, several times denser where they have points than that estimate: the k-th neighbour then
 * lies well inside one cell and the walk ends after shell 1 with a few times k candidates seen. */
#define SG_KNN_MAX_K 32
#define SG_KNN_MAX_SHELL 3
#define SG_KNN_FLAG_NOT_FINITE 1
#define SG_KNN_FLAG_CELL_RANGE 4
double sg_knn_default_cell(const double *lo, const double *hi, int64_t n, int k);
size_t sg_knn_workspace_bytes(int64_t n, int k);
int sg_knn(const float *xyz, int64_t n, int k, double cell, double max_dist, int32_t *idx, double *d2, int32_t *meta,
           void *ws, size_t ws_bytes, sg_stream_t stream);
/* NORMAL AND CURVATURE PER POINT.  nbr int32 [n, k] (1 <= k <= 4096, 0 <= n < 2^31, else SG_ERR_UNSUPPORTED): -1 =
 * no entry; an index outside -1 .. n - 1 is never dereferenced, counts as -1 and sets SG_GEOMETRY_FLAG_INDEX in
 * meta[1].  The support of point i is i itself followed by its valid neighbours in list order.  Centroid: the
 * double sum in that order divided by the count.  Covariance: the six double sums, in that order, of the products
 * of the centred coordinates (dx*dx, dx*dy, dx*dz, dy*dy, dy*dz, dz*dz; dx = (double)x - mean_x).  With T = (cxx +
 * cyy) + czz the point HAS NO NORMAL -- normal (0, 0, 0), curvature 0 -- when it has fewer than min_neighbours
 * valid neighbours or when not 0 < T < inf.  Otherwise the normal is the unit eigenvector of the smallest
 * eigenvalue l0, its sign such that the component of greatest magnitude is positive (the lowest axis among equal
 * magnitudes), and curvature = max(l0, 0) / (l0 + l1 + l2); both are rounded to float32 at the end.  The solver:
 * eight cyclic Jacobi sweeps in double on C / T.  meta int32 [4]: [0] = points without a normal, [1] = flags. */
#define SG_GEOMETRY_FLAG_INDEX 1
#define SG_GEOMETRY_FLAG_INTERNAL 2
int sg_point_normals(const float *xyz, int64_t n, const int32_t *nbr, int k, int min_neighbours, float *normals,
                     float *curvature, int32_t *meta, sg_stream_t stream);
/* GROWN SEGMENTS.  nbr int32 [n, k] as above, normals float32 [n, 3], curvature float32 [n] or NULL, nbr_d2 double
 * [n, k] (required when max_dist >= 0, else unused).  Entry m of point i's list, j = nbr[i][m], is a LINK between i
 * and j when both have a normal (a component that is not 0), fabs((nx_i*nx_j + ny_i*ny_j) + nz_i*nz_j) >= cos_thr
 * in double from the float32 normals, with curvature both curvatures <= max_curvature (float32 comparison), and
 * with max_dist >= 0 nbr_d2[i][m] <= max_dist * max_dist (double).  A segment is a connected component of the
 * links (an entry in either list links both ways).  Components of at least min_size (>= 1) points are numbered
 * 0 .. n_seg - 1 in ascending order of their smallest point; sp int32 [n] gets that number.  The other points get
 * -1, or with absorb = 1 the number of the first entry of their own list (list order) that lies in a numbered
 * component, else -1 -- one pass that reads only the labels from before the pass.
 * Lock-free union-find with parent[i] <= i (a find ends after n + 1 steps, a union after 2 n + 2 rounds; a bound
 * that is hit sets SG_GEOMETRY_FLAG_INTERNAL), sizes by integer atomicAdd at the roots, numbers by a scan over the
 * roots in index order.  meta int32 [4]: [0] = n_seg, [1] = flags, [2] = components of any size. */
size_t sg_grow_segments_workspace_bytes(int64_t n);
int sg_grow_segments(const int32_t *nbr, const double *nbr_d2, int64_t n, int k, const float *normals,
                     const float *curvature, double cos_thr, float max_curvature, double max_dist, int min_size,
                     int absorb, int32_t *sp, int32_t *meta, void *ws, size_t ws_bytes, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The object table of a mask list (csrc/objects.hip): per mask its population, axis-aligned box, centroid, centred
 * second moments, colour mean, the smallest enclosing rectangle over a table of yaw directions and the semantic
 * vote.  The reference has no counterpart.  Opt-in: nothing calls it unless asked.  softgroup_amd.ops.objects' numpy
 * twins are the definition; every entry equals them byte for byte, and two calls give the same bytes.  Arithmetic
 * is integer and IEEE double without contraction; no float atomics.
 *
 * INPUTS.  bits uint32 [n, ceil(N / 32)]: point i is bit i % 32 of word i / 32, bits at and beyond N are ignored.
 * coords float32 [N, 3]; colors float32 [N, 3] or NULL; semantic int32 or int64 [N].  0 <= n <= 16384 masks,
 * 0 <= N < 2^31 (else SG_ERR_UNSUPPORTED, nothing is launched).  flags int32 [1] is written by the entry: bit
 * SG_OBJECTS_FLAG_NOT_FINITE when a coordinate (or colour) of a point of at least one mask is not finite -- the
 * outputs then mean nothing; a value at a point that is in no mask is never read.
 *
 * 1. POPULATION AND BOX.  npoint[m] = the number of mask points; aabb[m] = (xmin, ymin, zmin, xmax, ymax, zmax) in
 *    double from the float32 coordinates.  EVERY extreme of this stage is canonicalised with + 0.0 (-0.0 -> +0.0).
 * 2. SUMS IN A FIXED ORDER.  The sum over the points of mask m of a double v(i): LEAF of word w: acc = +0.0, then
 *    acc = acc + v(32 w + b) for the set bits b in ascending order.  TREE: the leaves of words 0 .. W-1, padded with
 *    +0.0 to the next power of two, are added in adjacent pairs a'[k] = a[2k] + a[2k+1], level by level.  (A leaf is
 *    never -0.0, so an all-zero subtree may be skipped.)  sum_xyz[m] = the sums of (double)x, (double)y, (double)z;
 *    centroid = sum / (double)npoint; cov6[m] = the sums of (dx dx, dx dy, dx dz, dy dy, dy dz, dz dz), dx =
 *    (double)x - cx, each product one multiplication, each sum divided once by (double)npoint; mean_color[m] = the
 *    three colour sums divided by (double)npoint.
 * 3. YAW SWEEP.  table double [A, 2] (row_stride 0: one table for all masks) or [n, A, 2] (row_stride A): (c, s)
 *    per direction, 1 <= A <= 180.  Per mask point u = (double)x * c + (double)y * s, v = (double)y * c - (double)x
 *    * s (two products and one add or subtract each).  Per (mask, direction) umin, umax, vmin, vmax, each + 0.0;
 *    area = (umax - umin) * (vmax - vmin).  best_index[m] = the direction of the smallest area, the lowest index
 *    among equal areas; best_ext[m] = its (umin, umax, vmin, vmax).  all_ext double [n, A, 4], when not NULL, gets
 *    the four extremes of every direction (then the workspace is not used).
 * 6. SEMANTIC VOTE.  hist int32 [n, C], 1 <= C <= 256 (else SG_ERR_UNSUPPORTED): per mask the count of every label
 *    in 0 .. C-1 over its points, other values are not counted.  sem_label[m] = the class of the greatest count, the
 *    lowest among equal counts, sem_count[m] that count; -1 / 0 for a mask without a counted label.
 * 7. EMPTY MASKS.  npoint 0, every double output NaN, best_index -1, sem_label -1.
 * (4. refinement and 5. box composition are host code over these entries: softgroup_amd.util.objects.) */
#define SG_OBJECTS_FLAG_NOT_FINITE 1
size_t sg_instance_moments_workspace_bytes(int n, int64_t n_points);
int sg_instance_moments(const uint32_t *bits, int n, int64_t n_points, const float *coords, const float *colors,
                        int32_t *npoint, double *aabb, double *sum_xyz, double *centroid, double *cov6,
                        double *mean_color, int32_t *flags, void *ws, size_t ws_bytes, sg_stream_t stream);
size_t sg_instance_extents_workspace_bytes(int n, int n_angles);
int sg_instance_extents(const uint32_t *bits, int n, int64_t n_points, const float *coords, const double *table,
                        int row_stride, int n_angles, int32_t *best_index, double *best_ext, double *all_ext,
                        int32_t *flags, void *ws, size_t ws_bytes, sg_stream_t stream);
int sg_instance_class_hist(const uint32_t *bits, int n, int64_t n_points, const void *semantic, int is_i64,
                           int n_classes, int32_t *hist, int32_t *sem_label, int32_t *sem_count, sg_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Result clouds to images (csrc/render.hip): a z-buffered point splat over several views at once and the colour
 * lookup with optional eye-dome lighting.  The reference has no counterpart.  Opt-in: nothing calls it unless asked.
 * softgroup_amd.ops.render's numpy twins are the definition; both entries equal them byte for byte, and two calls
 * give the same bytes: a z-buffer is a minimum over integer keys, so the order of arrival does not matter.  No float
 * atomics; every operation below is ONE IEEE double operation, in the order written, without contraction; the device
 * evaluates no transcendental function.
 *
 * INPUTS.  coords float32 [N, 3].  cams double [V, SG_RENDER_CAMERA_DOUBLES], in device memory, one row per view:
 * [0] kind (0 perspective, 1 orthographic), [1..3] eye, [4..12] the rotation row-major with rows (right, up,
 * forward), [13] f, [14] cx, [15] cy, [16] 1 when near is given, [17] near, [18] 1 when far is given, [19] far.
 * The host computes all of it once, for both backends; a perspective camera needs near > 0.  Image width W, height
 * H, row 0 at the top.  Either point_size, the splat radius in pixels (0 .. 16), or world_radius w > 0 (then
 * point_size is ignored).  Range: 0 <= N < 2^31 - 1, 1 <= V <= 16, 1 <= W, H <= 8192, V H W <= 2^26 (else
 * SG_ERR_UNSUPPORTED, nothing is launched).
 *
 * RULES per (view, point i).
 *   dx = (double)x - ex, dy, dz likewise; xc = (r00 dx + r01 dy) + r02 dz, yc and zc from rows 1 and 2.
 *   Visible when zc >= near (near given) and zc <= far (far given); a comparison with NaN is false, so a coordinate
 *   that is not finite culls itself.
 *   perspective: u = cx + f (xc / zc), v = cy - f (yc / zc); orthographic: u = cx + f xc, v = cy - f yc.
 *   Culled unless -2^30 < u < 2^30 and -2^30 < v < 2^30, tested on the doubles before any conversion to an integer.
 *   px = floor(u), py = floor(v).
 *   r = point_size, or with w: perspective floor(f (w / zc)), orthographic floor(f w), clipped to 0 .. 16.
 *   The point covers the pixels (px + a, py + b), a, b = -r .. r, that lie inside the image (a splat across a border
 *   is clipped per pixel, not dropped).
 *   d = (float)zc + 0.0f; key = (ord32(d) << 32) | i, ord32 the order-preserving map of the float bits (all bits
 *   flipped for a negative value, the sign bit set otherwise).  The pixel's owner is the smallest key: the nearest
 *   depth after rounding to float32, the LOWEST point among equal depths.  All ones = empty.
 * index int32 [V, H, W] gets the owner (-1: empty), depth float32 [V, H, W] its d (+inf: empty), culled int32 [V]
 * the number of culled points of every view (not an error).  Emptiness is index < 0: a zc beyond the float32 range
 * rounds to d = +inf and the point still owns its pixel, with depth +inf.
 *
 * stages: SG_RENDER_STAGE_ALL, or for measurements the stages one by one on the same workspace, in this order: FILL
 * (keys [V, H, W] uint64 in the workspace to all ones, culled to 0), SPLAT (a lane per point, the views in an inner
 * loop; per covered pixel an 8-byte relaxed agent-scope load and a 64-bit atomicMin only when the key is smaller),
 * RESOLVE (a lane per pixel, keys to index / depth).
 *
 * SHADE.  image uint8 [V, H, W, 3]: the background for an empty pixel, colors[i] (uint8 [n_colors, 3]) for a pixel
 * owned by point i.  An owner outside 0 .. n_colors-1 is never dereferenced: the pixel gets the background and flags
 * int32 [1] gets SG_RENDER_FLAG_COLOR_INDEX.  With edl != 0 (strength >= 0, radius s in 1 .. 4, scale > 0) every
 * channel of an owned pixel of depth d is scaled: the eight neighbours at (dx, dy) s, (dx, dy) in the order
 * (-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1) (dy > 0 is down); a neighbour outside the
 * image is not counted; an empty one contributes 0; any other one t = (double)d - (double)dn, t = t > 0 ? t : 0,
 * t = t / scale, t = t < 1 ? t : 1.  resp = the sum in that order, from +0.0, divided by (double)count, or 0 when
 * count == 0; shade = 1.0 / (1.0 + strength resp); c' = (uint8)floor((double)c shade + 0.5). */
#define SG_RENDER_CAMERA_DOUBLES 20
#define SG_RENDER_FLAG_COLOR_INDEX 1
#define SG_RENDER_STAGE_FILL 1
#define SG_RENDER_STAGE_SPLAT 2
#define SG_RENDER_STAGE_RESOLVE 4
#define SG_RENDER_STAGE_ALL 7
size_t sg_render_rasterize_workspace_bytes(int n_views, int width, int height);
int sg_render_rasterize(const float *coords, int64_t n, const double *cams, int n_views, int width, int height,
                        int point_size, double world_radius, int stages, int32_t *index, float *depth,
                        int32_t *culled, void *ws, size_t ws_bytes, sg_stream_t stream);
int sg_render_shade(const int32_t *index, const float *depth, int n_views, int width, int height,
                    const uint8_t *colors, int64_t n_colors, int bg_r, int bg_g, int bg_b, int edl, double strength,
                    int radius, double scale, uint8_t *image, int32_t *flags, sg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SOFTGROUP_HIP_H */
