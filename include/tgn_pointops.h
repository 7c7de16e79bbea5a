/*
 * tgn_pointops.h -- C ABI of libtgn_pointops.so, the MI355X (gfx950) implementation of
 * ToothGroupNetwork's point-cloud sampling / grouping hot path.
 *
 * Plain pointers and sizes only (device pointers unless stated), no torch types.  The host
 * side (toothgroupnetwork_amd/_lib.py) binds these with ctypes and passes tensor.data_ptr()
 * and the current HIP stream.
 *
 * Section 1 re-exports, name for name and argument for argument, the `extern "C"` launchers the
 * reference's pybind layer binds (limhoyeon/ToothGroupNetwork, external_libs/pointops/src):
 * a maintainer can link the reference's *_cuda.cpp wrappers against this library unchanged.
 * They run on the stream set with tgn_set_default_stream() (the reference uses the null
 * stream, e.g. sampling_cuda_kernel.cu:136) and report errors through tgn_last_error().
 *
 * Section 2 holds the stream-aware forms of the same operators (trailing stream, int status)
 * and Section 3 the operators the reference composes out of torch kernels
 * (external_libs/pointnet2_utils/pointnet2_utils.py) that are single HIP kernels here.
 *
 * All functions are thread-safe as long as callers own their buffers; scratch is caller-provided.
 * Status: 0 = ok, non-zero = error (tgn_last_error() gives the text).  Layouts are row-major
 * contiguous fp32 / int32 exactly as the reference's kernels expect.
 */
#ifndef TGN_POINTOPS_H
#define TGN_POINTOPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *tgn_stream_t; /* a hipStream_t; NULL = the null stream */

#define TGN_OK 0
#define TGN_ERR_INVALID_ARGUMENT 1
#define TGN_ERR_LAUNCH 2
#define TGN_ERR_UNSUPPORTED 3

/* flags of tgn_furthestsampling* */
#define TGN_FPS_FMA 1         /* d = fma(dz,dz,fma(dy,dy,dx*dx)): nvcc's contraction of sampling_cuda_kernel.cu:54 */
#define TGN_FPS_LOCAL_INDEX 2 /* write indices relative to the cloud's first point (pointnet2_utils.py:96) */
#define TGN_FPS_INDEX64 4     /* idx is int64_t* instead of int32_t* */
#define TGN_FPS_TREE_TIES 8   /* equal distances resolved like the CUDA kernel's shared-memory tree (:5-10,64-123) */
#define TGN_FPS_CUDA_COMPAT (TGN_FPS_FMA | TGN_FPS_TREE_TIES)
#define TGN_FPS_LOW_VALU 16   /* scheduling hint, same results: clouds of 2048 - 4096 points also take the bucket-skipping kernel.
                                 Alone it is ~15 % slower there than the plain register-resident kernel, but it issues a tenth of
                                 the vector instructions -- the right choice when the launch runs beside ALU-bound work */

#define TGN_FPS_THROUGHPUT 32 /* scheduling hint, same results: clouds of 4 097 - 32 768 points run the owner-wave kernel out of a
                                 cell-sorted, L2-resident workspace (tgn_fps_throughput_workspace_bytes; the *_ws / *_prefix entry
                                 points) instead of out of registers: 58 VGPRs per lane, so FOUR workgroups share a CU where the
                                 register-resident kernel allows one.  A single cloud takes 1.5x as long; a batch of several
                                 clouds per CU finishes sooner (profiles/r06_fps_throughput.txt).  Ignored without a workspace. */

const char *tgn_version(void);
const char *tgn_last_error(void);     /* per host thread */
/* Stream of the section-1 entry points (which have no stream argument); per host thread, default NULL. */
void tgn_set_default_stream(tgn_stream_t stream);
/*
 * FPS arithmetic of furthestsampling_cuda_launcher (which has no flags argument): any of TGN_FPS_TREE_TIES |
 * TGN_FPS_FMA.  Process-wide; initialised from the environment (TGN_FPS_TIES=first|tree, TGN_FPS_FMA=0|1), default 0 =
 * first-index ties, unfused distance.  TGN_FPS_TREE_TIES reproduces the tie order of the reference kernel's
 * shared-memory tree (sampling_cuda_kernel.cu:5-10,64-123) and is pinned against that kernel (oracle/_ref).
 */
void tgn_set_fps_mode(int flags);
int tgn_get_fps_mode(void);
/*
 * Kernel-variant switches for A/B runs and the parity tests that must reach every kernel.  One table of atomics inside the
 * library, read with a relaxed load on the launch paths (no getenv there); the legacy TGN_* environment names seed it once,
 * when the library is loaded.  Thread-safe; a change applies to launches enqueued after the call.
 *   "fps_bucket_min"     smallest cloud the bucket kernel takes, -1 = built-in thresholds; values above 4097 act as 4097:
 *                        a cloud of more than 4096 points always takes the bucket kernel                (TGN_FPS_BUCKET_MIN)
 *   "fps_lean"           0 = no lean kernel, 1 = lean kernel for 257 .. 2048 points (default), 2 = up to 4096     (TGN_FPS_LEAN)
 *   "ball_bitmap"        0 = rank-select ball-query kernel, any other value = the chunked bitmap kernel (default 2)
 *                                                                                                        (TGN_BALL_BITMAP)
 *   "sa_tile"            0 = pick, 128 / 256 = force the workgroup tile of tgn_sa_mlp2_max_bf16x3                (TGN_SA_TILE)
 *   "gather_v4"          gather family: bit 0 forward kernels with 16-byte lanes, bit 2 subtraction / aggregation backward
 *                        with owner-side sums (default 5); other bits are ignored                      (TGN_GATHER_V4)
 * tgn_set_tuning returns TGN_ERR_INVALID_ARGUMENT for an unknown key; tgn_get_tuning returns `fallback` for one.
 */
int tgn_set_tuning(const char *key, int value);
int tgn_get_tuning(const char *key, int fallback);

/* ------------------------------------------------------------------------------------------
 * 1. The reference's C ABI, verbatim (each line cites the declaration it replaces).
 * ---------------------------------------------------------------------------------------- */
/* sampling/sampling_cuda_kernel.h:13 ; n = max points per cloud ; tmp (n_total) pre-filled 1e10 */
void furthestsampling_cuda_launcher(int b, int n, const float *xyz, const int *offset, const int *new_offset,
                                    float *tmp, int *idx);
/* knnquery/knnquery_cuda_kernel.h:13 ; dist2 = squared distances, ascending */
void knnquery_cuda_launcher(int m, int nsample, const float *xyz, const float *new_xyz, const int *offset,
                            const int *new_offset, int *idx, float *dist2);
/* grouping/grouping_cuda_kernel.h:14-15 ; grad_input (n,c) pre-zeroed, accumulated into */
void grouping_forward_cuda_launcher(int m, int nsample, int c, const float *input, const int *idx, float *output);
void grouping_backward_cuda_launcher(int m, int nsample, int c, const float *grad_output, const int *idx,
                                     float *grad_input);
/* interpolation/interpolation_cuda_kernel.h:14-15 ; output / grad_input pre-zeroed, accumulated into */
void interpolation_forward_cuda_launcher(int n, int c, int k, const float *input, const int *idx,
                                         const float *weight, float *output);
void interpolation_backward_cuda_launcher(int n, int c, int k, const float *grad_output, const int *idx,
                                          const float *weight, float *grad_input);
/* subtraction/subtraction_cuda_kernel.h:14-15 ; grad_input1 / grad_input2 (n,c) pre-zeroed, accumulated into */
void subtraction_forward_cuda_launcher(int n, int nsample, int c, const float *input1, const float *input2,
                                       const int *idx, float *output);
void subtraction_backward_cuda_launcher(int n, int nsample, int c, const int *idx, const float *grad_output,
                                        float *grad_input1, float *grad_input2);
/* aggregation/aggregation_cuda_kernel.h:14-15 ; output (n,c) and the three gradients pre-zeroed: the kernels add to what they
 * find there, as the reference's do (aggregation_cuda_kernel.cu:18,35-37) */
void aggregation_forward_cuda_launcher(int n, int nsample, int c, int w_c, const float *input,
                                       const float *position, const float *weight, const int *idx, float *output);
void aggregation_backward_cuda_launcher(int n, int nsample, int c, int w_c, const float *input,
                                        const float *position, const float *weight, const int *idx,
                                        const float *grad_output, float *grad_input, float *grad_position,
                                        float *grad_weight);

/* ------------------------------------------------------------------------------------------
 * 2. Stream-aware forms of the same operators.
 * ---------------------------------------------------------------------------------------- */
/*
 * Farthest point sampling over b packed clouds (pointops.py:10-27).  n_max = largest cloud.
 * tmp may be NULL unless a cloud exceeds tgn_fps_resident_capacity() points (then it must hold
 * offset[b-1] floats; contents on entry are ignored; the dense form: B * N floats).  new_xyz (m,3) is optional (NULL to skip): the
 * sampled coordinates, i.e. xyz[idx] (pointnet2_utils.py:276 / blocks.py:70).
 */
int tgn_furthestsampling(int b, int n_max, const float *xyz, const int *offset, const int *new_offset,
                         float *tmp, void *idx, float *new_xyz, int flags, tgn_stream_t stream);
/* Dense batch (B,N,3) -> (B,S): the offsets of pointnet2_utils.py:87-96 are implicit. */
int tgn_furthestsampling_dense(int B, int N, int S, const float *xyz, float *tmp, void *idx, float *new_xyz,
                               int flags, tgn_stream_t stream);
int tgn_fps_resident_capacity(void);
/*
 * The order in which the bucket-skipping FPS kernel deals a cloud's grid cells out to its buckets: out[x | y << bits |
 * z << 2 * bits] = position of cell (x, y, z) along the kernel's space-filling curve (a Hilbert curve; bits = 4, 4096
 * entries).  Host memory, no device needed: for tools/fps_bucket_model.py and the tests of the mapping.
 */
int tgn_fps_bucket_order(int bits, unsigned short *out);
/*
 * Clouds larger than tgn_fps_resident_capacity() (raw scans, preprocess_data.py:55-56) run the bucket-skipping
 * kernel out of a cell-sorted workspace of tgn_fps_workspace_bytes(b, n_max) bytes (20 B per point; 0 when every
 * cloud fits the register-resident kernels; clouds above 262 144 points fall back to streaming through the same
 * buffer used as the reference's tmp array, which then must hold 4 B per point of the batch).
 */
size_t tgn_fps_workspace_bytes(int b, int n_max);
/* Workspace of the TGN_FPS_THROUGHPUT form (20 B per point, whatever the cloud size up to 32 768 points; 0 above). */
size_t tgn_fps_throughput_workspace_bytes(int b, int n_max);
int tgn_furthestsampling_ws(int b, int n_max, const float *xyz, const int *offset, const int *new_offset,
                            void *workspace, size_t workspace_bytes, void *idx, float *new_xyz, int flags,
                            tgn_stream_t stream);
int tgn_furthestsampling_dense_ws(int B, int N, int S, const float *xyz, void *workspace, size_t workspace_bytes,
                                  void *idx, float *new_xyz, int flags, tgn_stream_t stream);
/*
 * FPS of an FPS result is the identity: if a cloud IS the sequence p_0, p_1, ... produced by farthest point sampling
 * (canonical first-index tie order, same arithmetic flags), sampling it again returns positions 0, 1, 2, ... -- which
 * is what the reference's set-abstraction / transition-down chains compute at every level after the first
 * (pointnet2_utils.py:160 on the previous level's new_xyz; blocks.py:69-70).  It holds as long as every winning
 * distance of the producing run was > 0 and < 1e10 (no exhausted cloud, no NaN/Inf point); the winning distance never
 * increases, so the first and the last one decide.
 *   prefix_out[b] (int32 per cloud, optional): this result's samples 0 .. prefix_out[b]-1 carry the property -- the
 *                 requested sample count when the run stayed inside (0, 1e10), 1 (nothing claimed) otherwise.
 *   prefix_in[b]  (int32 per cloud, optional): cloud b of xyz is such a sequence up to prefix_in[b] samples; when that
 *                 covers the requested sample count (and TGN_FPS_TREE_TIES is not set) the kernel writes the identity
 *                 (indices, new_xyz, prefix_out) and returns -- decided on the device, per cloud, no host sync.
 * The caller vouches for provenance: prefix_in must come from the prefix_out of the launch that produced xyz.
 * prefix_ref (optional, same layout as xyz): the new_xyz that launch wrote; the kernel then takes the shortcut for a
 * cloud only if its coordinates equal prefix_ref bit for bit -- provenance by content, for callers that cannot
 * vouch for it (the model gathers p[idx] itself, blocks.py:70, or hands tensors through arbitrary code).
 */
int tgn_furthestsampling_prefix(int b, int n_max, const float *xyz, const int *offset, const int *new_offset,
                                void *workspace, size_t workspace_bytes, void *idx, float *new_xyz, const int *prefix_in,
                                const float *prefix_ref, int *prefix_out, int flags, tgn_stream_t stream);
int tgn_furthestsampling_dense_prefix(int B, int N, int S, const float *xyz, void *workspace, size_t workspace_bytes,
                                      void *idx, float *new_xyz, const int *prefix_in, const float *prefix_ref,
                                      int *prefix_out, int flags, tgn_stream_t stream);

/* kNN (pointops.py:30-45): b segments; idx (m,nsample) int32; dist2 (m,nsample) squared, ascending. */
int tgn_knnquery(int b, int m, int nsample, const float *xyz, const float *new_xyz, const int *offset,
                 const int *new_offset, int *idx, float *dist2, tgn_stream_t stream);
/*
 * Same result, ~30x faster: with tgn_knnquery_workspace_bytes(m) bytes of device scratch the wave-parallel
 * kernel runs first and only queries whose k+1 smallest distances tie bit-for-bit are redone by the exact
 * heap kernel (whose insertion history decides the order of tied neighbours, knnquery_cuda_kernel.cu:21-48).
 */
size_t tgn_knnquery_workspace_bytes(int m);
int tgn_knnquery_ws(int b, int m, int nsample, const float *xyz, const float *new_xyz, const int *offset,
                    const int *new_offset, int *idx, float *dist2, void *workspace, size_t workspace_bytes,
                    tgn_stream_t stream);
/*
 * The same result again through per-segment uniform grids (cell size ~ the k-neighbour radius of a scan surface): a
 * query looks at the 3x3x3 cells around it instead of the whole segment and widens the block only if the (k+1)-th
 * distance does not lie inside the covered radius.  n = total number of points (rows of xyz).  Pays from a few
 * thousand points per segment up; small or degenerate segments are scanned linearly inside the same launch, and
 * nsample > 63 or too small a workspace fall back to tgn_knnquery_ws.  (24 000 x 24 000, k = 36: see DESIGN.md.)
 */
size_t tgn_knnquery_grid_workspace_bytes(int b, int n, int m);
int tgn_knnquery_grid(int b, int n, int m, int nsample, const float *xyz, const float *new_xyz, const int *offset,
                      const int *new_offset, int *idx, float *dist2, void *workspace, size_t workspace_bytes,
                      tgn_stream_t stream);

int tgn_grouping_forward(int m, int nsample, int c, const float *input, const int *idx, float *output,
                         tgn_stream_t stream);
int tgn_grouping_backward(int m, int nsample, int c, const float *grad_output, const int *idx, float *grad_input,
                          tgn_stream_t stream);
int tgn_interpolation_forward(int n, int c, int k, const float *input, const int *idx, const float *weight,
                              float *output, tgn_stream_t stream);
int tgn_interpolation_backward(int n, int c, int k, const float *grad_output, const int *idx, const float *weight,
                               float *grad_input, tgn_stream_t stream);
int tgn_subtraction_forward(int n, int nsample, int c, const float *input1, const float *input2, const int *idx,
                            float *output, tgn_stream_t stream);
int tgn_subtraction_backward(int n, int nsample, int c, const int *idx, const float *grad_output,
                             float *grad_input1, float *grad_input2, tgn_stream_t stream);
int tgn_aggregation_forward(int n, int nsample, int c, int w_c, const float *input, const float *position,
                            const float *weight, const int *idx, float *output, tgn_stream_t stream);
int tgn_aggregation_backward(int n, int nsample, int c, int w_c, const float *input, const float *position,
                             const float *weight, const int *idx, const float *grad_output, float *grad_input,
                             float *grad_position, float *grad_weight, tgn_stream_t stream);

/*
 * Point-Transformer vector attention (models/modules/cbl_point_transformer/blocks.py:31-44), packed layout.
 *
 * tgn_pt_attention_forward: the whole PointTransformerLayer after its three input projections, eval mode:
 *     p_r = linear_p(p[idx] - p)                      Linear(3,3) + BatchNorm1d(3) folded into (Wp1, bp1), ReLU, Linear(3,c) = (Wp2, bp2)
 *     w   = linear_w(x_k[idx] - x_q + p_r)            BatchNorm1d(c) as (a1, t1), ReLU, Linear(c,g) + BatchNorm1d(g) folded into
 *                                                     (Ww1, bw1), ReLU, Linear(g,g) = (Ww2, bw2);  g = c / share_planes
 *     out = sum_j (x_v[idx_j] + p_r_j) * softmax_j(w)[.., ch % g]
 *   p (n,3), x_q / x_k / x_v (n,c), idx (n,nsample) int32 neighbour rows (the kNN of p among p), out (n,c).
 *   post_scale / post_shift (c each, or both NULL): out = relu(out * post_scale + post_shift) -- the BatchNorm + ReLU the block
 *   applies to the layer's output (blocks.py:151), folded.
 *   One kernel, nothing of size n*nsample*c is written.  nsample <= 64, c % 4 == 0, g in {4,8,16,32,64}.
 * tgn_pt_softmax_aggregate_{forward,backward}: the trainable tail alone (blocks.py:41-43): softmax over the
 *   neighbours of logit (n,nsample,g) -> sm (kept for backward), out[n,ch] = sum_j (x_v[idx[n,j],ch] + p_r[n,j,ch]) *
 *   sm[n,j,ch % g]; the backward writes grad_pr (n,nsample,c), grad_logit (n,nsample,g) and ACCUMULATES into grad_xv
 *   (n_v,c; pre-zeroed).  This is the reference's `aggregation` (aggregation_cuda_kernel.cu:5-39) with the softmax
 *   fused in front.  grad_xv == NULL: the scatter is left out (a kernel instantiation without it) and nothing is written for it;
 *   the caller sums grad_pr along reverse lists instead (tgn_scatter_ordered below).
 */
int tgn_pt_attention_forward(int n, int nsample, int c, int g, const float *p, const float *xq, const float *xk,
                             const float *xv, const int *idx, const float *Wp1, const float *bp1, const float *Wp2,
                             const float *bp2, const float *a1, const float *t1, const float *Ww1, const float *bw1,
                             const float *Ww2, const float *bw2, const float *post_scale, const float *post_shift, float *out,
                             tgn_stream_t stream);
int tgn_pt_softmax_aggregate_forward(int n, int nsample, int c, int g, const float *xv, const float *pr, const float *logit,
                                     const int *idx, float *sm, float *out, tgn_stream_t stream);
int tgn_pt_softmax_aggregate_backward(int n, int nsample, int c, int g, const float *xv, const float *pr, const float *sm,
                                      const int *idx, const float *grad_out, float *grad_xv, float *grad_pr,
                                      float *grad_logit, tgn_stream_t stream);

/*
 * The gather family's backward without float atomics (csrc/scatter_ordered.hip): a scatter-add out[idx[q]] += term(q) turned
 * round, so that one lane group owns an output row and adds that row's terms in a fixed order.  The same inputs give the same
 * bits.  Both calls launch on `stream` and neither allocate, copy, nor synchronise: they can be captured in a graph.
 *
 *   tgn_reverse_lists: idx holds b * pairs_per_batch indices (int32, or int64 with idx_is64); pair q = bi * pairs_per_batch + t
 *     targets row bi * n + idx[q]; an index outside [0, n) counts as row 0 of its batch.  rev_start (b * n + 1) and rev_pair
 *     (b * pairs_per_batch) int32: rev_pair[rev_start[r] .. rev_start[r + 1]) holds the pair numbers that target row r in ascending
 *     order, rev_start[b * n] = b * pairs_per_batch.  The packed operators call it with b = 1, the dense layout with its B, N and
 *     S * K.  Every entry of both outputs is written; `ws` (device memory, at least tgn_reverse_lists_workspace_bytes bytes, any
 *     contents) is free again when the call has run.  b * n and b * pairs_per_batch must be below 2^31 (else
 *     TGN_ERR_INVALID_ARGUMENT with a message, and the size function returns 0).  Integer atomics only; a segment longer than 64
 *     pairs is sorted by one workgroup in len^2 / 256 steps per thread: slow for a row that very many pairs target, bounded, exact.
 *
 *   tgn_scatter_ordered: out (n_rows, c); out[r][ch] is the float32 sum, starting from +0.0f and taken sequentially in list order
 *     over the pairs q of row r, of term(q, ch); every term is rounded to float32 before it is added and nothing is contracted.
 *       coef == NULL (pair rows):   term = sign * src[q * c + ch]                                  src (pairs, c)
 *       coef != NULL (query rows):  term = (sign * src[(q / k) * c + ch]) * coef[q * g + ch % g]   src (pairs / k, c), coef (pairs, g),
 *                                                                                                   g dividing c
 *     sign is +1 or -1, k >= 1.  The pairs of row r are rev_pair[rev_start[r] .. rev_start[r + 1]) -- lists as tgn_reverse_lists
 *     writes them; they are trusted: an entry is a pair number of src / coef -- or, with rev_start == NULL and rev_pair == NULL,
 *     the identity segments r * k .. r * k + k - 1.  Every element of out is written (a row without pairs gets +0.0f): the caller
 *     does not pre-zero it.
 */
size_t tgn_reverse_lists_workspace_bytes(int b, int n, long long pairs_per_batch);
int tgn_reverse_lists(int b, int n, long long pairs_per_batch, const void *idx, int idx_is64, int *rev_start, int *rev_pair,
                      void *ws, size_t ws_bytes, tgn_stream_t stream);
int tgn_scatter_ordered(long long n_rows, int c, int k, int g, const int *rev_start, const int *rev_pair, const float *src,
                        const float *coef, float sign, float *out, tgn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 3. pointnet2_utils operators as single kernels (dense (B,N,*) layout).
 * ---------------------------------------------------------------------------------------- */
/* square_distance (pointnet2_utils.py:20-41) for 3-D points: src (B,N,3), dst (B,M,3) -> out (B,N,M). */
int tgn_square_distance(int B, int N, int M, const float *src, const float *dst, float *out, tgn_stream_t stream);
/*
 * query_ball_point (pointnet2_utils.py:120-144): first nsample indices in ascending index order with
 * square_distance(new_xyz, xyz) <= r2 (expanded-form arithmetic of pointnet2_utils.py:20-41), padded
 * with the first hit; a row without any hit is filled with N.  idx: (B,S,nsample) int32 or int64.
 * workspace: tgn_ball_query_workspace_bytes(B,N,S) bytes of device scratch (may be NULL if 0).
 */
size_t tgn_ball_query_workspace_bytes(int B, int N, int S);
int tgn_ball_query(int B, int N, int S, int nsample, float r2, const float *xyz, const float *new_xyz, void *idx,
                   int idx_is_int64, void *workspace, size_t workspace_bytes, tgn_stream_t stream);
/*
 * The same in two launches, for planners: _build fills the workspace (per-cloud uniform grid: depends on xyz and r2 only,
 * not on the queries -- it can run while the sampling that produces new_xyz is still in flight), _prebuilt answers the
 * queries from a workspace filled by _build with the same (B, N, S, nsample, r2, xyz).  Same results as tgn_ball_query.
 */
/* out[r, 0..ncols) = in[r, first..first+ncols) for `rows` rows of `stride` floats: the xyz block of (N, 6) scan rows
 * (gen_utils.py:138, pointnet_pp_model.py:16-20) without torch's strided-copy kernel (10x slower beside a running FPS launch) */
int tgn_slice_columns(long long rows, int stride, int first, int ncols, const float *in, float *out, tgn_stream_t stream);
/* scheduling spacer: a one-wave kernel that idles for about `microseconds` on `stream` (planners: hold one stream's work
 * back behind another's start without a host round trip) */
int tgn_stream_delay(int microseconds, tgn_stream_t stream);
int tgn_ball_query_build(int B, int N, int S, int nsample, float r2, const float *xyz, void *workspace,
                         size_t workspace_bytes, tgn_stream_t stream);
int tgn_ball_query_prebuilt(int B, int N, int S, int nsample, float r2, const float *xyz, const float *new_xyz, void *idx,
                            int idx_is_int64, void *workspace, size_t workspace_bytes, tgn_stream_t stream);
/*
 * Grouping of sample_and_group (pointnet2_utils.py:162-169, xyz_first=1: [xyz[idx]-new_xyz, points[idx]])
 * and of PointNetSetAbstractionMsg (pointnet2_utils.py:281-285, xyz_first=0: [points[idx], xyz[idx]-new_xyz]).
 * points (B,N,D) may be NULL (D ignored).  out: (B,S,K,3+D).
 */
int tgn_group_points(int B, int N, int S, int K, int D, const float *xyz, const float *new_xyz, const float *points,
                     const void *idx, int idx_is_int64, int xyz_first, float *out, tgn_stream_t stream);
/*
 * The same with the launch knobs exposed.  impl: 0 = choose, 1 = 4-B stores, 2 = 16-B stores through LDS (needs
 * K*(3+D) % 4 == 0).  store_policy: cache-policy bits of the 16-B output stores (0 plain, 2 nt, 16 sc1 = write-through,
 * the output lines do not stay in L2; -1 = the kernel's default: nt for the LDS-image kernels, sc1 for the others).  max_blocks: upper bound on the grid (0 = none) for callers
 * that overlap the grouping with a kernel that needs most of every CU (the FPS level-1 workgroups).
 */
int tgn_group_points_ex(int B, int N, int S, int K, int D, const float *xyz, const float *new_xyz,
                        const float *points, const void *idx, int idx_is_int64, int xyz_first, float *out, int impl,
                        int store_policy, int max_blocks, tgn_stream_t stream);
/*
 * The three kernels of the fused set-abstraction level (eval mode, BatchNorm folded; pointnet2_utils.py:229-236,
 * 281-294).  With scale = gamma/sqrt(var+eps), shift = beta - mean*scale and W = the first 1x1 convolution:
 *
 * tgn_sa_point_transform: A[m,:] = [points[m,:], xyz[m,:]] * Wt for the M = B*N points of a batch -- the per-POINT half
 *   of the layer (the convolution commutes with the gather).  Wt: (D+3, C1) row-major, rows ordered
 *   [feature channels..., x, y, z], columns already multiplied by scale.  Hand-written fp32-MFMA GEMM
 *   (v_mfma_f32_32x32x2_f32: exact fp32 fma chain).
 * tgn_sa_gather_max: out[b,s,c] = act( max_k A[b, idx[b,s,k], c] - (Wxs[0,c]*cx + Wxs[1,c]*cy + Wxs[2,c]*cz) + b2[c] )
 *   with (cx,cy,cz) = new_xyz[b,s], Wxs = the x,y,z rows of Wt, b2 = shift + scale*bias: the whole single-layer
 *   set-abstraction level, (B,S,C1) out, nothing of size S*K written.  nsample <= 64, C1 % 4 == 0.
 * tgn_sa_direct_max: the same result without the per-point tensor for narrow inputs (3+D <= 16, C1 % 32 == 0,
 *   C1 <= 256, nsample <= 64; tgn_sa_direct_supported): a wave owns a query and contracts its K gathered rows
 *   [x-c, f] (D+3) with Wd on the matrix cores.  Wd: (16, C1), rows [x, y, z, f0.., zero padding], scale folded.
 */
int tgn_sa_point_transform(long long M, int D, int C1, const float *xyz, const float *points, const float *Wt, float *A,
                           tgn_stream_t stream);
int tgn_sa_gather_max(int B, int N, int S, int K, int C1, const float *A, const float *new_xyz, const float *Wxs,
                      const float *b2, const void *idx, int idx_is_int64, int relu, float *out, tgn_stream_t stream);
/* First layer of a MULTI-layer shared MLP: out[b,s,k,c] = act(A[b,idx[b,s,k],c] - Wxs[:,c].centre + b2[c]), (B,S,K,C1). */
int tgn_sa_gather_act(int B, int N, int S, int K, int C1, const float *A, const float *new_xyz, const float *Wxs,
                      const float *b2, const void *idx, int idx_is_int64, int relu, float *out, tgn_stream_t stream);
int tgn_sa_direct_supported(int K, int D, int C1);
int tgn_sa_direct_max(int B, int N, int S, int K, int D, int C1, const float *xyz, const float *new_xyz,
                      const float *points, const float *Wd, const float *b2, const void *idx, int idx_is_int64, int relu,
                      float *out, tgn_stream_t stream);
/*
 * tgn_sa_mlp2_max: a WHOLE set-abstraction level with a TWO-layer shared MLP (what every level of the reference networks
 * has: pointnet_pp.py:13-15, tsg_centroid_module.py:10-12, tsg_seg_module.py:11-28), eval mode, both BatchNorms folded:
 *   out[b,s,:] = max_k relu(W2 * relu(W1 * [x[idx]-c, f[idx]] + b1) + b2)        (pointnet2_utils.py:281-294)   (B,S,C2)
 * in ONE kernel: neither the grouped tensor nor the (B,S,K,C1) / (B,S,K,C2) layer outputs are written.  The second layer
 * runs on the fp32 matrix cores (exact fp32).  First layer, two forms:
 *   commuted (A1 != NULL): A1 (B,N,C1p) = tgn_sa_point_transform of the level's points with the first layer's folded
 *     weights; W1 = Wxs (3,C1p), the x,y,z rows of those weights; xyz / points unused (may be NULL);
 *   direct (A1 == NULL, 3+D <= 16; tgn_sa_mlp2_direct_supported): W1 = Wd (16,C1p), rows [x, y, z, f0.., zero padding].
 * C1p = the first layer's width padded with zero columns to a multiple of 16 (b1, W1, A1 padded alike);
 * W2f (C1p/8, C2, 8): W2f[kb][c][i] = scale2[c] * W2[c, 8*kb + i] (zero for padded k); b2 (C2) = shift2 + scale2*bias2.
 * nsample <= 64; idx int32 or int64, local to each cloud, out-of-range handled like tgn_group_points.
 * out_stride: floats between consecutive rows of `out` (0 = C2): a multi-scale level lets every (radius, nsample) branch write
 * its columns of the concatenated (B,S,sum C2) tensor directly (pointnet2_utils.py:296-298 concatenates them).
 */
int tgn_sa_mlp2_direct_supported(int K, int D);
int tgn_sa_mlp2_max(int B, int N, int S, int K, int D, int C1p, int C2, const float *A1, const float *xyz,
                    const float *points, const float *new_xyz, const float *W1, const float *b1, const void *idx,
                    int idx_is_int64, const float *W2f, const float *b2, float *out, int out_stride, tgn_stream_t stream);
/*
 * The same level with the second layer on the BF16 matrix cores at fp32 accuracy ("bf16x3").  v_mfma_f32_32x32x16_bf16 runs at
 * 16x the rate of the fp32-input MFMA; both operands are written as sums of three bf16 numbers (24 mantissa bits) and a product is
 * six bf16 MFMAs with fp32 accumulation -- a1 b1 + a1 b2 + a2 b1 + a2 b2 + a1 b3 + a3 b1, the dropped terms are below 2^-24 of the
 * product -- i.e. fp32-class rounding at up to 16 / 6 = 2.7x the fp32-MFMA rate.  Not bit-identical to tgn_sa_mlp2_max; held to the
 * same elementwise 1e-5 bound against the float64 oracle.
 *   tgn_sa_mlp2_split_bytes(C1p, C2)    size of the split weight image;
 *   tgn_sa_mlp2_split_weights           W2f (C1p/8, C2, 8) fp32 -> image (device to device, once per weight matrix): per 128-column
 *                                       tile and 16-wide K tile the 12 KiB the kernel's LDS tile holds, fetched by LDS-DMA;
 *   tgn_sa_mlp2_max_bf16x3              tgn_sa_mlp2_max with W2s (the image) in place of W2f; every other argument as above.
 */
size_t tgn_sa_mlp2_split_bytes(int C1p, int C2);
/* tgn_sa_point_transform on the same scheme: Wts = tgn_sa_mlp2_split_weights(Kp, C1, Wtf) with Wtf (Kp/8, C1, 8),
 * Wtf[kb][c][i] = Wt[8 kb + i][c] (rows [features..., x, y, z], zero rows past D + 3), Kp = D + 3 rounded up to a multiple of 16. */
int tgn_sa_point_transform_bf16x3(long long M, int D, int Kp, int C1, const float *xyz, const float *points, const void *Wts,
                                  float *A, tgn_stream_t stream);
int tgn_sa_mlp2_split_weights(int C1p, int C2, const float *W2f, void *W2s, tgn_stream_t stream);
int tgn_sa_mlp2_max_bf16x3(int B, int N, int S, int K, int D, int C1p, int C2, const float *A1, const float *xyz,
                           const float *points, const float *new_xyz, const float *W1, const float *b1, const void *idx,
                           int idx_is_int64, const void *W2s, const float *b2, float *out, int out_stride, tgn_stream_t stream);
/*
 * tgn_sa_all_mlp2_max: PointNetSetAbstraction with group_all=True -- the only form of that module a reference model builds
 * (models/modules/tsg_seg_module.py:28: 515 -> [256, 512] over the 256 points of the last level) -- eval mode, BatchNorms folded:
 *   out[b,:] = max_n relu(W2 * relu(W1 * [x_n, f_n] + b1) + b2)     (pointnet2_utils.py:178-195 + 229-236)     (B,C2)
 * The whole cloud is one group, there is no centre and no index tensor: chunks of 64 consecutive points run through the
 * two-layer kernel of tgn_sa_mlp2_max, a second small launch takes the maximum over a cloud's chunks.  Operands as for
 * tgn_sa_mlp2_max, with the group_all channel order [x, y, z, features] (pointnet2_utils.py:190): commuted form A1 (B,N,C1p) =
 * tgn_sa_point_transform (Wd unused, may be NULL), direct form A1 == NULL with xyz, points, Wd (16,C1p).
 * part: workspace of tgn_sa_all_chunks(N) * B * C2 floats (may be NULL when tgn_sa_all_chunks(N) == 1).
 */
int tgn_sa_all_chunks(int N);
int tgn_sa_all_mlp2_max(int B, int N, int D, int C1p, int C2, const float *A1, const float *xyz, const float *points,
                        const float *Wd, const float *b1, const float *W2f, const float *b2, float *part, float *out,
                        int out_stride, tgn_stream_t stream);
/*
 * Weight gradient of a linear layer with few columns and many (or not so many) rows -- the training path of the Point-Transformer
 * mirrors; blocks.py:19-30 declares the layers:
 *   dW[o][i] = sum_r gy[r][o] * x[r][i]      (cout, cin)         db[o] = sum_r gy[r][o]   (optional, NULL to skip)
 * a contraction over the ROWS with a small result, which the BLAS libraries walk with one or two tiles (94 us for a 256 x 256
 * gradient over 375 rows).  One wave per (row slice, 32 x 32 output tile) on the fp32 matrix cores straight from global memory,
 * then one reduction over the slices.  x (rows, cin), gy (rows, cout), row-major fp32; workspace of
 * tgn_linear_wgrad_workspace_bytes(rows, cin, cout) bytes.
 */
size_t tgn_linear_wgrad_workspace_bytes(long long rows, int cin, int cout);
int tgn_linear_wgrad(long long rows, int cin, int cout, const float *x, const float *gy, float *dW, float *db, void *workspace,
                     size_t workspace_bytes, tgn_stream_t stream);

/*
 * Training-mode BatchNorm1d over the rows of x (rows, C), optionally fused with the ReLU that follows it: the normalisations of
 * the Point-Transformer training path (blocks.py:37,40 via nn.BatchNorm1d; this package normalises the flattened (n * nsample, c)
 * rows).  forward: batch statistics in double, y = [relu]((x - mean) * invstd * gamma + beta), save_mean / save_invstd for the
 * backward pass, running statistics updated like nn.BatchNorm1d (running = (1 - momentum) running + momentum batch, variance
 * unbiased; NULL running pointers: not tracked), *num_batches_tracked += 1 when given.  backward: dx, dgamma, dbeta; with relu
 * the mask is y > 0 (y = the forward output).  workspace: tgn_bn_rows_workspace_bytes(C) bytes, ZERO before the first use -- the
 * kernels leave it zeroed, so one buffer serves every call of a layer on one stream.  rows >= 2, 1 <= C <= 1024, fp32, contiguous.
 */
size_t tgn_bn_rows_workspace_bytes(int C);
int tgn_bn_rows_forward(long long rows, int C, const float *x, const float *gamma, const float *beta, float eps, float momentum,
                        float *running_mean, float *running_var, long long *num_batches_tracked, int relu, float *y,
                        float *save_mean, float *save_invstd, void *workspace, tgn_stream_t stream);
int tgn_bn_rows_backward(long long rows, int C, const float *x, const float *y, const float *dy, const float *gamma,
                         const float *save_mean, const float *save_invstd, int relu, float *dx, float *dgamma, float *dbeta,
                         void *workspace, tgn_stream_t stream);
/*
 * The same two calls with ORDERED reductions: no float or double atomic (and no integer one either), so every output has the same
 * bits on every call, whatever else runs on the device.  Operands, limits and status codes as above, plus workspace_bytes: less
 * than tgn_bn_rows_ordered_workspace_bytes(rows, C) (0 for unsupported rows / C) is TGN_ERR_INVALID_ARGUMENT before any launch.
 * The workspace may hold ANYTHING on entry (as for tgn_reverse_lists) and holds the partial sums afterwards; calls that share one
 * must be ordered on one stream.  Three launches per call, no host synchronisation, capturable.
 * The summation order is a function of (rows, C) only.  With total = rows * C, m = C / gcd(256, C) and
 * B = min(1024, max(1, ceil(total / 8192))) rounded up to a multiple of m, the reduction runs B blocks of 256 threads, T = 256 B:
 *   1. thread t = 256 b + i adds the terms of elements t, t + T, t + 2 T, ... (all in column t % C) in ascending order from +0.0.
 *      forward: s1 += (double)x, s2 += (double)x * (double)x.  backward, with g = dy (0 where relu and y <= 0) and all of
 *      g * ((x - mean) * invstd) in float: s1 += (double)g, s2 += (double)that product;
 *   2. in block b the thread i < min(C, 256) adds to its own sums those of threads i + C, i + 2 C, ... < 256, ascending: the block's
 *      partial for column (256 b + i) % C.  A column none of its threads keeps (C > 256) gets +0.0;
 *   3. per column, chain j < 64 adds the partials of blocks j, j + 64, j + 128, ... in ascending order from +0.0;
 *   4. the chains j = 0 .. min(B, 64) - 1 are added in ascending order from +0.0.
 * All sums are double, the library is built with -ffp-contract=off, and what follows is the arithmetic of the atomic form: mean =
 * s1 / rows, var = max(0, s2 / rows - mean * mean), invstd = 1 / sqrt(var + eps), the running statistics in double with var * (rows /
 * (rows - 1)), dbeta = (float)s1, dgamma = (float)s2.  tests/bn_ordered_ref.py restates all of it in numpy.
 */
size_t tgn_bn_rows_ordered_workspace_bytes(long long rows, int C);
int tgn_bn_rows_forward_ordered(long long rows, int C, const float *x, const float *gamma, const float *beta, float eps,
                                float momentum, float *running_mean, float *running_var, long long *num_batches_tracked, int relu,
                                float *y, float *save_mean, float *save_invstd, void *workspace, size_t workspace_bytes,
                                tgn_stream_t stream);
int tgn_bn_rows_backward_ordered(long long rows, int C, const float *x, const float *y, const float *dy, const float *gamma,
                                 const float *save_mean, const float *save_invstd, int relu, float *dx, float *dgamma, float *dbeta,
                                 void *workspace, size_t workspace_bytes, tgn_stream_t stream);
/* index_points (pointnet2_utils.py:44-61): out[b,j,:] = points[b, idx[b,j], :], idx flattened to (B,M). */
int tgn_gather_points(int B, int N, int M, int C, const float *points, const void *idx, int idx_is_int64, float *out,
                      tgn_stream_t stream);
/* backward of tgn_gather_points / tgn_group_points feature part: grad_points[b, idx[b,j], :] += grad_out[b,j,:] */
int tgn_scatter_add_points(int B, int N, int M, int C, const float *grad_out, const void *idx, int idx_is_int64,
                           float *grad_points, tgn_stream_t stream);
/*
 * three nearest support points (pointnet2_utils.py:333-335): xyz1 (B,N,3) queries, xyz2 (B,S,3) support;
 * dist (B,N,3) expanded-form squared distances ascending by (dist, index); idx int32 or int64.
 */
int tgn_three_nn(int B, int N, int S, const float *xyz1, const float *xyz2, float *dist, void *idx, int idx_is_int64,
                 tgn_stream_t stream);
/* inverse-distance weighted sum (pointnet2_utils.py:337-340); weight (B,N,3) is also written if non-NULL. */
int tgn_three_interpolate(int B, int N, int S, int C, const float *points2, const float *dist, const void *idx,
                          int idx_is_int64, float *out, float *weight, tgn_stream_t stream);
/* the same with the epilogue of the eval-mode feature propagation fused in (pointnet2_utils.py:337-347, first convolution
 * commuted onto the coarse points): out = [relu](interpolation (+ add)); add (B,N,C) may be NULL and may be `out` itself. */
int tgn_three_interpolate_ex(int B, int N, int S, int C, const float *points2, const float *dist, const void *idx,
                             int idx_is_int64, const float *add, int relu, float *out, float *weight, tgn_stream_t stream);
/*
 * Gather indices follow torch's advanced indexing (pointnet2_utils.py:56-60): negative values wrap (k + N); an
 * index still outside [0,N) -- where the reference raises, e.g. an empty ball yields index N -- makes
 * tgn_gather_points write a zero row and tgn_group_points / tgn_sa_* read point 0, and latches a flag in the
 * current device's memory -- one flag per (device, stream), so host threads that drive different streams do not see or
 * clear each other's.  This returns the word and clears it -- 1 (bit 0) if that happened in a launch on `stream` since the last
 * call, 2 (bit 1) for what the crop and clustering entry points below latch, 0 for neither; it synchronises `stream`.  (The Python
 * operators call it and raise IndexError.)
 */
int tgn_take_index_error(tgn_stream_t stream);
/* The same over every stream of the current device (synchronises the DEVICE, ORs and clears all of its flags): for planners
 * that launch unchecked on streams of their own (HotPath), graphs replayed on another stream than they were captured on
 * (a graph keeps the capture stream's flag), and TGN_INDEX_CHECK=off sections. */
int tgn_take_index_error_device(void);
/* Clears the flag in stream order without synchronising: what a checked operator issues in front of its own launch, so
 * that a bit latched by an earlier UNCHECKED launch is not attributed to it. */
int tgn_clear_index_error(tgn_stream_t stream);

/*
 * The crop step between the two stages of tgnet_fps's GroupingNetworkModule (models/modules/grouping_network_module.py:45-72, on the
 * labelled path): per-label centroids, the k nearest points of every centroid, the centred crops.  The reference runs it on the host
 * (numpy, an sklearn KDTree, python gathers).  feats (b, c_stride, n) channel-first float32 with xyz in channels 0..2; labels (b, n) int64.
 *   tgn_label_centroids: counts (b, nlab) int32 and cent (b, nlab, 3) float32 over the labels 0..nlab-1 (-1 = gingiva is skipped), cent
 *     bit-equal to numpy's xyz[label == t].mean(axis=0): a sequential float32 sum in point order divided by the count (NaN for an absent
 *     label).  1 <= nlab <= 64.  A label outside [-1, nlab) is ignored and latches bit 1 of the stream's error word (tgn_take_index_error).
 *   tgn_label_centroids_f64: the same counts, and cent from a float64 sum in point order, divided by the count and rounded to float32
 *     once: the mean itself to half an ulp, where the float32 sum above drifts with the number of points (the training losses' centroids).
 *   tgn_crop_knn: for crop t (centroid cent (t_total, 3), scan crop_scan[t]) the k nearest points of that scan, idx_out (t_total, k)
 *     int64, ascending in the float64 squared distance ((0 + dx*dx) + dy*dy) + dz*dz (dx = double(x) - double(cx), unfused: sklearn's
 *     euclidean rdist on KDTree's float64 copy), equal distances by ascending point index (KDTree leaves their order unspecified).
 *     1 <= k <= min(n, 4096).  A crop_scan value outside [0, b) latches bit 1 and writes index 0.
 *   tgn_crop_gather_center: out (t_total, c, k) = feats[crop_scan[t]][:, idx[t]] with channels 0..2 minus their mean over the k points
 *     (float64 sum in a fixed order, the mean rounded once to float32, subtracted in float32: ops_utils.centering_object); out_labels
 *     (t_total, 1, k) int64 = labels[crop_scan[t]][idx[t]] with every value >= 0 set to 0 (NULL: not written).  An index outside [0, n)
 *     reads point 0 and latches bit 1.
 * Deterministic: no atomic whose order reaches an output.  t_total = 0 launches nothing.
 */
int tgn_label_centroids(int b, int n, int c_stride, const float *feats, const long long *labels, int nlab, int *counts, float *cent,
                        tgn_stream_t stream);
int tgn_label_centroids_f64(int b, int n, int c_stride, const float *feats, const long long *labels, int nlab, int *counts, float *cent,
                            tgn_stream_t stream);
int tgn_crop_knn(int b, int n, int c_stride, const float *feats, int t_total, const int *crop_scan, const float *cent, int k,
                 long long *idx_out, tgn_stream_t stream);
int tgn_crop_gather_center(int b, int n, int c, int t_total, int k, const float *feats, const int *crop_scan, const long long *idx,
                           const long long *labels, float *out, long long *out_labels, tgn_stream_t stream);

/*
 * The clustering of tgnet_fps's unlabelled path (ops_utils.get_clustering_labels, called from grouping_network_module.py:57-69): sklearn's
 * DBSCAN and flat-kernel MeanShift on the moved foreground points, the moments of its PCA split test, the noise points' vote.  The
 * reference runs it on the host.  q is a neighbour of p within radius r when ((0 + dx*dx) + dy*dy) + dz*dz <= r*r in float64, unfused
 * (dx = double(p.x) - double(q.x): KDTree's euclidean rdist, as tgn_crop_knn); the point itself and exact duplicates count.
 *   tgn_dbscan: DBSCAN(eps, min_samples).fit(X) on each of b clouds of xyz (n, 3) float32 row-major, cloud i = points
 *     [offset[i-1], offset[i]) (pointops-style cumulative int32 offset (b), device memory, offset[b-1] = n; not checked here).  core (n)
 *     uint8: 1 when the neighbour count (self included) is >= min_samples.  labels (n) int64, numbered per cloud: the connected
 *     components of core points under the neighbour relation are clusters 0, 1, ... in ascending order of their smallest core index
 *     (sklearn's dbscan_inner); a non-core point with a core neighbour takes the smallest of its core neighbours' cluster numbers
 *     (the first depth-first search of dbscan_inner that reaches it), every other point is noise (-1).  nclusters (b) int32.  eps > 0,
 *     min_samples >= 1.  workspace: at least tgn_dbscan_workspace_bytes(b, n) bytes of device memory, O(n).
 *   tgn_mean_shift: MeanShift(bandwidth)'s climb (_mean_shift_single_seed, max_iter iterations at most; sklearn's default is 300) from
 *     every point of xyz (n, 3) float64: the new mean is the sum of the points within the bandwidth, sequential in ascending point order
 *     from -0.0 (the identity of IEEE addition: the sum is p0 + p1 + ... and nothing else; numpy's axis-0 sum is the same sum started from
 *     +0.0, bit-equal except that a column of nothing but -0.0 gives +0.0 there), divided by their count; a seed stops when the shift's
 *     norm is <= 1e-3 * bandwidth or max_iter steps were completed before this one (max_iter = 0: one step).  means (n, 3) float64 the
 *     final mean, counts (n)
 *     int32 the number of points it is the mean of (0: no point within the bandwidth, the seed stayed where it was).  sklearn sums in
 *     its KDTree's order instead, so the means agree with sklearn's to rounding, not bit for bit.
 *   tgn_nearest_center: labels (n) int64 = the index of the centre (m, 3) float64 nearest to each point of xyz (n, 3) float64, by rdist,
 *     ties to the lower index.  m >= 1.
 *   tgn_cluster_moments: for every label l in [0, nlab): counts (nlab) int32 of the points i with labels[i] == l and mask[i] != 0 (mask
 *     NULL: all), their float64 mean (nlab, 3) and covariance (nlab, 3, 3) with ddof = 1.  Fewer than 2 points: every covariance entry is
 *     NaN (as np.cov); no point: count 0 and the mean is NaN too.  xyz (n, 3) float32.
 *   tgn_cluster_vote: out[i] = the most frequent of cand_labels[nn_idx[i][0..k-1]], equal counts to the smallest label (np.unique +
 *     argmax).  1 <= k <= 32.  An index outside [0, n_cand) reads candidate 0 and latches bit 1 of the stream's error word.
 * Deterministic: no atomic whose order reaches an output.  n = 0 (m = 0 for the vote) launches nothing where it is allowed.
 */
size_t tgn_dbscan_workspace_bytes(int b, int n);
int tgn_dbscan(int b, int n, const float *xyz, const int *offset, double eps, int min_samples, long long *labels, unsigned char *core,
               int *nclusters, void *workspace, size_t workspace_bytes, tgn_stream_t stream);
int tgn_mean_shift(int n, const double *xyz, double bandwidth, int max_iter, double *means, int *counts, tgn_stream_t stream);
int tgn_nearest_center(int n, const double *xyz, int m, const double *centers, long long *labels, tgn_stream_t stream);
int tgn_cluster_moments(int n, const float *xyz, const long long *labels, const unsigned char *mask, int nlab, int *counts, double *mean,
                        double *cov, tgn_stream_t stream);
int tgn_cluster_vote(int m, int k, const long long *nn_idx, int n_cand, const long long *cand_labels, long long *out, tgn_stream_t stream);

/*
 * The join between the two stages of tsegnet (models/modules/tsegnet.py:57-81) and the painting loop of its inference pipeline
 * (inference_pipelines/inference_pipeline_tsegnet.py:60-66); the reference runs both on the host.  Between tgn_tsg_proposals and
 * tgn_tsg_crop_features lie tgn_dbscan, tgn_label_centroids and tgn_crop_knn.
 *   tgn_tsg_proposals: for each scan s of b, l3_xyz, offset (b, 3, m) and dist (b, 1, m) float32 channel-first: point j is kept when
 *     dist[s, 0, j] < threshold in float32 (NaN is dropped); moved[row] = l3_xyz[s, :, j] + offset[s, :, j], one float32 addition per
 *     coordinate.  The kept points are written to moved (b * m, 3) row-major PACKED: scan after scan, ascending j inside a scan, the
 *     first sum(counts) rows; counts (b) int32 the kept points per scan.  1 <= m <= 1024.  One workgroup per scan, no atomics.
 *     Meant for the b of a forward (b small): every workgroup recounts the scans in front of it, b * (b - 1) / 2 * m comparisons in all.
 *   tgn_tsg_crop_features: for crop t (scan crop_scan[t], centre cent[t], indices idx (t_total, k) int64): out (t_total, 3 + cf + 1, k)
 *     float32 with channels 0..2 = feats[scan][0..2, idx] (feats (b, c_stride, n), xyz first; bit copies, NOT centred), channels
 *     3..3+cf-1 = l0_points[scan][:, idx] (l0_points (b, cf, n); bit copies; cf = 0: none, l0_points may be NULL), the last channel =
 *     expf(-4 * sqrtf(d)) with d = ((-2 * dot(p, c)) + |p|^2) + |c|^2 in float32, the expanded form of square_distance
 *     (pointnet2_utils.py:20-41; dot = fma(pz, cz, fma(py, cy, px * cx)), |v|^2 = ((x*x) + (y*y)) + (z*z), as tgn_square_distance).  d is
 *     NOT clamped: where it rounds below zero the feature is NaN, exactly where the reference's torch.sqrt gives NaN.  out_labels
 *     (t_total, 1, k) int64 = labels[scan][idx] unchanged (labels (b, n) int64; NULL out_labels: not written).  A crop_scan value
 *     outside [0, b) reads scan 0, an index outside [0, n) reads point 0; both latch bit 1 of the stream's error word.
 *   tgn_tsg_paint: out (b, n) int64: out[s, p] = ids[t*], t* the LARGEST crop number t with crop_scan[t] = s that holds p = idx[t, pos]
 *     at a position with mask[t, pos] != 0 (mask (t_total, k) uint8, ids (t_total) int64), and 0 where no crop does: the result of
 *     writing the crops one after the other in ascending t.  Entries with a scan outside [0, b) or an index outside [0, n) are skipped
 *     and latch bit 1.  t_total = 0: out is zeroed.
 * Deterministic: no atomic whose order reaches an output (tgn_tsg_paint takes an integer maximum).  t_total = 0 launches nothing.
 * The cluster means in between come from tgn_label_centroids, whose limit is 64 labels: a scan whose proposals form more than 64
 * clusters (256 proposals with min_samples = 3 allow up to 85) is refused by the host layer, where the reference would go on.
 * t_total <= 65535.
 */
int tgn_tsg_proposals(int b, int m, const float *l3_xyz, const float *offset, const float *dist, float threshold, float *moved,
                      int *counts, tgn_stream_t stream);
int tgn_tsg_crop_features(int b, int n, int c_stride, int cf, int t_total, int k, const float *feats, const float *l0_points,
                          const int *crop_scan, const float *cent, const long long *idx, const long long *labels, float *out,
                          long long *out_labels, tgn_stream_t stream);
int tgn_tsg_paint(int b, int n, int t_total, int k, const int *crop_scan, const long long *idx, const unsigned char *mask,
                  const long long *ids, long long *out, tgn_stream_t stream);

/*
 * The geometric training losses as fused kernels (csrc/loss.hip), forward and backward.  All tensors float32 and contiguous unless
 * said otherwise; offset, xyz (b, 3, n) channel-first.  Squared distances are the direct form ((dx*dx) + (dy*dy)) + (dz*dz) in float32;
 * every sum that crosses threads is float64 in a fixed order (wave, LDS, per-block partials in `workspace`, a finishing kernel) and
 * is rounded to float32 once.  No atomics on floats: the same inputs give the same bits.  The calls launch on `stream` and neither
 * allocate, copy nor synchronise; `workspace` (device memory, at least *_workspace_bytes) is free again when the forward has run.
 *
 *   tgn_offset_loss_forward: batch_center_offset_loss and batch_chamfer_distance_loss of tgnet_fps (models/tgn_loss.py:6-61, 263-302).
 *     labels (b, n) int64 in -1..15 (-1 = gingiva; another value counts as gingiva and latches bit 1 of the stream's error word),
 *     counts (b, 16) int32 and cent (b, 16, 3) the per-tooth point counts and centroids of tgn_label_centroids_f64 (or tgn_label_centroids) with nlab = 16.  A tooth
 *     is valid when its count is >= 5.  With m = p + o, c_t the centroid of the point's tooth:
 *       losses[0] = (sum over valid (s, t) of (sum_i |m_i - c_t|^2) / n_st) / #valid
 *       losses[1] = (sum over valid (s, t) with k_st > 0 of (sum over kept i of (d_i . o_i/|o_i| - 1)^2) / k_st) / #those,
 *                   d = (c_t - p)/|c_t - p|, a point kept when |o| > 0.0002, k_st the kept points
 *       losses[2] = (1 / b) sum_s (sum over points with label != -1 of d1 / d2) / #those, d1 <= d2 the two smallest |m - c|^2 over the
 *                   VALID teeth of the scan
 *     An empty denominator gives NaN (0 / 0, as the reference); a scan with fewer than two valid teeth gives NaN for losses[2]
 *     (the reference raises).  scales (b, 33) receives what the backward needs: per tooth 1 / (n_st #valid) and 1 / (k_st #those),
 *     then 1 / (b #foreground); 0 where the term is undefined.
 *   tgn_offset_loss_backward: grad_offset (b, 3, n) = grad_losses[0] d losses[0] + grad_losses[1] d losses[1] + grad_losses[2] d losses[2]
 *     with respect to offset (grad_losses: 3 floats in DEVICE memory).  A point the direction term does not keep, an exactly zero
 *     offset included, gets a zero direction gradient (the reference's autograd gives NaN for an exact zero); a term whose loss is
 *     NaN for want of teeth contributes zero.
 *
 *   tgn_centroid_loss_forward: centroid_loss of tsegnet (models/tsg_loss.py:4-61).  offset, xyz (b, 3, m), distance (b, m), centroid
 *     (b, 3, c) with 1 <= c <= 16, exists (b, c) bytes or NULL (every centroid exists); absent centroids are skipped in both
 *     directions.  With m_j = x_j + o_j, d1 <= d2 the two smallest |m_j - c|^2, g_c = min_j |c - m_j|^2 over the scan's points:
 *       losses[0] = mean over b m of smooth_l1(distance - sqrt(min_c |x - c|^2)), beta 1
 *       losses[1] = sum(d1 | distance <= 0.2) / # + sum(g_c | g_c <= 0.2) / #        (counts over the whole batch)
 *       losses[2] = sum(d1 / d2 | d1 <= 0.2) / #
 *     An empty mask gives NaN; fewer than two existing centroids in a scan give NaN for losses[2].  scales (4) and rev_arg (b, 16)
 *     int32 (the argmin of every g_c that is <= 0.2, lowest index on a tie, else -1) are for the backward.
 *   tgn_centroid_loss_backward: grad_offset (b, 3, m) and grad_distance (b, m) for grad_losses (3 floats in device memory).  Every
 *     point collects the reverse term by looking for its own index among its scan's 16 saved argmins: one launch, no atomics.
 */
size_t tgn_offset_loss_workspace_bytes(int b, int n);
int tgn_offset_loss_forward(int b, int n, const float *offset, const float *xyz, const long long *labels, const int *counts,
                            const float *cent, float *losses, float *scales, void *workspace, size_t ws_bytes, tgn_stream_t stream);
int tgn_offset_loss_backward(int b, int n, const float *offset, const float *xyz, const long long *labels, const int *counts,
                             const float *cent, const float *scales, const float *grad_losses, float *grad_offset, tgn_stream_t stream);
size_t tgn_centroid_loss_workspace_bytes(int b);
int tgn_centroid_loss_forward(int b, int m, int c, const float *offset, const float *xyz, const float *distance, const float *centroid,
                              const unsigned char *exists, float *losses, float *scales, int *rev_arg, void *workspace, size_t ws_bytes,
                              tgn_stream_t stream);
int tgn_centroid_loss_backward(int b, int m, int c, const float *offset, const float *xyz, const float *distance, const float *centroid,
                               const unsigned char *exists, const float *scales, const int *rev_arg, const float *grad_losses,
                               float *grad_offset, float *grad_distance, tgn_stream_t stream);

/*
 * One decoder stage of the contrastive-boundary criterion (heads.ContrastHead.point_contrast) as fused kernels (csrc/cbl.hip), for
 * neighbour lists the caller supplies.  The (m, k1, c) tensor of latent differences is never formed.  f (m, c) float32, 16-byte
 * aligned; idx (m, k1) int32, the neighbour lists WITHOUT their column 0 (k1 = nsample - 1); labels (m) int64.  Sizes: 1 <= k1 <= 63,
 * c a multiple of 4 with 4 <= c <= 128, m * k1 < 2^31; anything else is TGN_ERR_UNSUPPORTED naming the value, before the first HIP
 * call.  m = 0: the forward writes loss = 0 and count = 0, the backward writes nothing.  An index outside [0, m) reads point 0 and
 * latches bit 0 of the stream's error word, as in the gather family.  The calls launch on `stream` and neither allocate, copy nor
 * synchronise; no atomics on floats: the same inputs give the same bits.  `workspace` (device memory, at least
 * tgn_cbl_stage_workspace_bytes(m), which grows by one step per 16 points) is free again when the forward has run.
 *
 *   tgn_cbl_stage_forward: for point i and slot j < k1, all in float32 with every operation rounded:
 *       s_q  = sum over the channels ch = q (mod 4), in channel order, of (f[i][ch] - f[idx[i][j]][ch])^2, from 0        (q = 0..3)
 *       d_ij = sqrtf(((s_0 + s_1) + (s_2 + s_3)) + 1e-12)                   e_ij = expf(min_j d_ij - d_ij)
 *       neg_i = sum_j e_ij, pos_i = sum_j e_ij [labels[idx[i][j]] == labels[i]]: butterflies over the 64 lanes of a wave (lane = slot,
 *               the lanes j >= k1 hold 0), lane distances 32, 16, .., 1
 *       r_i = pos_i / neg_i; the point contributes when 0 < #{j: labels[idx[i][j]] == labels[i]} < k1, with the value -logf(r_i + 1e-12)
 *     count (1) int64 = the number of contributing points; loss (1) = 0.1 * (sum of their values) / max(count, 1), the sum in float64
 *     (a workgroup's 16 points in point order, lane l of the finishing wave the workgroups l, l + 64, .., then a butterfly), rounded
 *     to float32 once.  pair_w (m, k1) = e_ij ([labels equal] - r_i) / ((neg_i (r_i + 1e-12)) d_ij) for a contributing point, exactly
 *     0 for every other row: dL_i / dd_ij divided by d_ij.
 *   tgn_cbl_stage_backward: grad_f (m, c), every row stored exactly once, zeros included:
 *       grad_f[i] = s (sum_j pair_w[i][j] (f[i] - f[idx[i][j]]) - sum over q in rev(i) of pair_w[q] (f[q / k1] - f[i]))
 *       s = (grad_loss[0] * 0.1) / max(count, 1) in float32                              (grad_loss: 1 float in DEVICE memory)
 *     rev(i) = the pair numbers q = i' k1 + j with idx[i'][j] == i, ascending, as rev_pair[rev_start[i] .. rev_start[i + 1]) with
 *     rev_start (m + 1) and rev_pair (m k1) int32.  Per channel in float32: from 0, the own pairs in slot order (acc = acc + w * diff),
 *     then the listed pairs in list order (acc = acc - w * diff), then s * acc.  A pair whose pair_w is exactly 0 is skipped, its rows
 *     unread.  A list entry outside [0, m k1) is skipped and latches the error word.
 */
size_t tgn_cbl_stage_workspace_bytes(int m);
int tgn_cbl_stage_forward(int m, int k1, int c, const float *f, const int *idx, const long long *labels, float *loss, long long *count,
                          float *pair_w, void *workspace, size_t ws_bytes, tgn_stream_t stream);
int tgn_cbl_stage_backward(int m, int k1, int c, const float *f, const int *idx, const float *pair_w, const long long *count,
                           const int *rev_start, const int *rev_pair, const float *grad_loss, float *grad_f, tgn_stream_t stream);

/*
 * DGCNN's neighbourhood work (models/modules/dgcnn.py).  x (B, D, N) float32 channel-first, as the network holds it.
 *   tgn_feature_knn: knn(x, k) (dgcnn.py:4-10) without the N x N matrix.  idx (B, N, k) int64 point indices local to their scan;
 *     row i holds the k smallest distances to point i, i itself included, in ascending (distance, index) order.  The distance is
 *     the direct form in float32 with every operation rounded: acc = 0; for c = 0..D-1: t = x[c][i] - x[c][j]; acc = acc + t*t.
 *     dist2 (B, N, k) float32 receives those distances (NULL: not written).  The result depends on the input alone (splitting
 *     and merging are exact).  Equal distances come in ascending index order, so a duplicate vertex of lower index precedes i
 *     (torch.topk leaves the order of equal values unspecified).  1 <= D <= 64, 1 <= k <= min(N, 32).  workspace: at least
 *     tgn_feature_knn_workspace_bytes(B, N, k) bytes of device memory (0: none needed), O(B N k).
 *   tgn_edgeconv2_max: out[b, coff + c, i] = max_{r < K} lrelu((W2 lrelu(P[b, idx[b,i,r]] + Q[b, i]) + b2)[c]), c = 0..63 -- an
 *     EdgeConv level of two 1x1 convolutions in eval mode with BatchNorm folded: P = Wa' x, Q = (Wb' - Wa') x + b1' per point
 *     (W' = the first layer's weight scaled by its BatchNorm, [Wa | Wb] its halves for [x_j - x_i, x_i]).  P, Q (B, N, 64) float32
 *     point-major, idx (B, N, K) int64, W2 (64, 64) float32 (out, in) row-major, b2 (64), lrelu = LeakyReLU(0.2).  The second layer
 *     runs on fp32 MFMA (exact fp32 products, fp32 accumulation).
 *   tgn_edgeconv1_max: out[b, coff + c, i] = max_{r < K} lrelu(P[b, idx[b,i,r], c] + Q[b, i, c]), the one-layer level.
 *   Both: out (B, *, N) float32 channel-first with batch stride ostride >= (coff + 64) * N floats, a buffer of at least
 *   (B - 1) * ostride + (coff + 64) * N floats; only channels coff .. coff + 63 of every scan are written; 1 <= K <= 32.  An index outside
 *   [0, N) reads point 0 and latches bit 1 of the stream's error word (tgn_take_index_error).
 */
size_t tgn_feature_knn_workspace_bytes(int B, int N, int k);
int tgn_feature_knn(int B, int N, int D, int k, const float *x, long long *idx, float *dist2, void *workspace, size_t ws_bytes,
                    tgn_stream_t stream);
int tgn_edgeconv2_max(int B, int N, int K, const float *P, const float *Q, const long long *idx, const float *W2, const float *b2,
                      float *out, long long ostride, int coff, tgn_stream_t stream);
int tgn_edgeconv1_max(int B, int N, int K, const float *P, const float *Q, const long long *idx, float *out, long long ostride, int coff,
                      tgn_stream_t stream);

/*
 * A pointwise linear layer fused with the max over the points: PointNet's stn.conv3, fstn.conv3 and feat.conv3
 * (pointnet_utils.py:29-32, 69-72, 127-128) and DGCNN's conv6 (dgcnn.py:117-118) in eval mode, without the (B, C, N) tensor.
 *   out[b, c] = max_{n < N} act( (sum_{k < K} x[b, k, n] * Wt[k, c]) + shift[c] )
 * x (B, K, N) float32 channel-first with rows of N contiguous floats; Wt (K, C) row-major with the BatchNorm scale folded into its
 * columns; shift (C) the folded bias and BatchNorm shift; act 0 = identity, 1 = relu, 2 = leaky relu with `slope`; out (B, C).
 * The sum is the fp32 MFMA's fma chain over k ascending from 0, shift is added once after it, the activation comes before the max.
 * A NaN candidate gives NaN (torch.max).  The max is exact, so scan b's result depends neither on B nor on how the launch cuts N:
 * bit equality.  Two launches (partial maxima per point chunk into ws, then their reduction), no float atomics, no allocation, no
 * synchronisation: capturable.  B, N, C >= 1 and 1 <= K <= 512; ws: at least tgn_linear_act_max_workspace_bytes(B, N, K, C) bytes
 * of device memory (0 for a shape that is refused).
 */
size_t tgn_linear_act_max_workspace_bytes(int B, int N, int K, int C);
int tgn_linear_act_max(int B, int N, int K, int C, const float *x, const float *Wt, const float *shift, int act, float slope,
                       float *out, void *ws, size_t ws_bytes, tgn_stream_t stream);

/*
 * Scoring a predicted segmentation against its ground truth: the reference's cal_metric (eval_visualize_results.py:20-57), which runs
 * about ten full-length numpy passes per predicted instance on the host.  Here the vertices are read once, into two integer tables per
 * scan, and the scores are computed from the tables.  Labels are int64; 2 <= nlab <= 64 (FDI numbers reach 48), anything else is
 * TGN_ERR_UNSUPPORTED with a message before any HIP call.
 *   tgn_seg_confusion_chunk: the number of vertices one workgroup of tgn_seg_confusion takes per pass (tests size their edge cases from it).
 *   tgn_seg_confusion: b scans packed end to end, n vertices in all, scan i = vertices [offset[i-1], offset[i]) (pointops-style cumulative
 *     int32 offset (b), device memory, as tgn_dbscan takes it; an empty scan is allowed; a vertex at or beyond offset[b-1] belongs to
 *     no scan; whatever offset holds, no access leaves the arrays).  ins_gt and ins_sem (b, nlab, nlab) int32: ins_gt[i][p][g] is the
 *     number of vertices of scan i with ins == p and gt == g, ins_sem[i][p][s] the number with ins == p and sem == s.  The call zeroes
 *     both tables itself, in stream order.  A vertex whose gt, sem or ins lies outside [0, nlab) is left out of BOTH tables and latches
 *     bit 1 of the stream's error word (tgn_take_index_error), as tgn_label_centroids does.  sem and ins may be the same array.
 *     0 <= n < 2^31; b = 0 does nothing, n = 0 zeroes the tables and launches nothing.
 *   tgn_seg_confusion_logits: the same tables, (B, C, C), for a semantic network's output with the argmax fused in.  logits (B, C, N)
 *     channel-first float32, 2 <= C <= 64.  A vertex's prediction is torch.argmax over its C logits: equal values go to the lowest
 *     channel, a NaN counts as larger than every number and the first NaN wins.  The prediction is both sem and ins; gt (B, N) int64 is
 *     counted as gt + gt_shift (the loaders hand gingiva as -1: callers pass 1).  A vertex whose shifted gt lies outside [0, C) is
 *     left out and latches bit 1.  B <= 65535.
 *   tgn_seg_scores: one workgroup per scan.  With A = ins_gt[i], S = ins_sem[i], n = sum(A), insc[p] = sum_g A[p][g] and
 *     gtc[g] = sum_p A[p][g]: for every p = 1 .. nlab-1 with insc[p] > 0, ascending, g = the first maximum of row A[p] and s = the first
 *     maximum of row S[p] (np.unique + argmax: ties to the smallest label), TP = A[p][g], FP = insc[p] - TP, FN = gtc[g] - TP,
 *     TN = n - TP - FP - FN, and in float64, unfused: acc += (TP+TN)/(FP+TP+FN+TN); prec = TP/(TP+FP); rec = TP/(TP+FN);
 *     f1 += (2*(prec*rec))/(prec+rec); iou += TP/(FP+TP+FN); sem_acc += 1 when s == g, or when is_half and s + 8 == g.  The sums run
 *     sequentially in ascending p and are divided by the number of instances at the end.  scores (b, 4) float64 = IoU, F1, ACC,
 *     SEM_ACC, bit-equal to the reference's; instances (b) int32 = the number of labels p >= 1 that occur; iou_per_instance (b, nlab)
 *     float64 (NaN where p is absent or 0); matched_gt (b, nlab) int32 = g (-1 where p is absent or 0).  A scan without an instance
 *     gives four NaN and instances = 0.
 * Deterministic: the only atomics are integer adds.  The calls neither allocate nor synchronise.
 */
int tgn_seg_confusion_chunk(void);
int tgn_seg_confusion(int b, long long n, const int *offset, const long long *gt, const long long *sem, const long long *ins, int nlab,
                      int *ins_gt, int *ins_sem, tgn_stream_t stream);
int tgn_seg_confusion_logits(int B, int C, int N, const float *logits, const long long *gt, int gt_shift, int *ins_gt, int *ins_sem,
                             tgn_stream_t stream);
int tgn_seg_scores(int b, int nlab, const int *ins_gt, const int *ins_sem, int is_half, double *scores, int *instances,
                   double *iou_per_instance, int *matched_gt, tgn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 4. Mesh input of the preprocess path (HOST pointers, CPU code): gen_utils.read_txt_obj_ls (gen_utils.py:207-233).
 * ---------------------------------------------------------------------------------------- */
/*
 * Text-OBJ reader with the reference loop's semantics (gen_utils.py:211-226), quirks included.  The contract, which the native
 * code meets on an ASCII subset and a Python loop (preprocess.read_obj) on everything else:
 *   - the file is opened as text: a line ends at "\n", "\r\n" or a lone "\r";
 *   - each line is split on white space; reading stops at the first line without a token (an empty or blank line);
 *   - only lines whose first token is exactly "v" or "f" count;
 *   - "v": float() of tokens 1..3 (further tokens are ignored);
 *   - "f": tokens 1..3; if the first holds "//", each is cut at its first "//"; then int().  Indices stay 1-based as in the file;
 *   - whatever float() / int() / the final array build reject is an error (TGN_ERR_INVALID_ARGUMENT natively, ValueError in Python).
 * The native subset: bytes below 0x80 only, in the whole file (behind the blank line that ends the read too); white space = space,
 * \t \n \v \f \r and \x1c - \x1f (what str.split() splits ASCII on); no '_' in a parsed token (Python takes "1_0"); coordinate tokens
 * of at most 400 and face references of at most 60 characters; three tokens behind every "v" and "f".  float() spellings taken
 * natively: sign, decimal and exponent forms, "inf" / "infinity" / "nan" in any letter case -- not hex, not "nan(...)".
 * A text outside the subset is TGN_ERR_UNSUPPORTED (tgn_last_error names the line and the reason), never a guess: the caller runs
 * the contract above in Python.  vertices (cap_v,3) double, faces (cap_f,3) int64.  tgn_obj_count reports exactly the counts
 * tgn_obj_read then delivers.
 */
int tgn_obj_count(const char *path, long long *n_vertices, long long *n_faces);
int tgn_obj_read(const char *path, double *vertices, long long *faces, long long cap_v, long long cap_f,
                 long long *n_vertices, long long *n_faces);
/*
 * Vertex normals as open3d's compute_vertex_normals() (gen_utils.py:228-233): area-weighted sum of the triangle
 * cross products, normalised, (0,0,1) where undefined.  triangles are ZERO-based.  Parity unpinned (no open3d here).
 */
int tgn_vertex_normals(const double *vertices, long long nv, const long long *triangles, long long nf, double *normals);
/*
 * One pass of open3d's TriangleMesh::SubdivideMidpoint (what the inference pipelines do to a mesh below 24 000 vertices,
 * inference_pipeline_sem.py:25-26), on the GPU: unlike its neighbours in this section it takes DEVICE pointers and a stream.
 * vertices (nv,3) double, normals (nv,3) double or NULL, triangles (nf,3) int64 ZERO-based.  The triangles are walked in order and,
 * per triangle (a, b, c), the edges (a,b), (b,c), (c,a); an edge is the unordered pair {min, max}.  The first time an edge is met it
 * gets vertex nv + (number of distinct edges met before it) = 0.5 * (V[p] + V[q]), with normal 0.5 * (N[p] + N[q]) (not renormalised)
 * when normals are given; triangle t becomes (a, ab, ca), (ab, b, bc), (bc, c, ca), (ab, bc, ca) at rows 4t .. 4t+3.  Old vertices keep
 * their indices and bits; a repeated index (a == b) is no special case (the edge {a, a} gets a copy of V[a]); unreferenced vertices
 * are kept.  The contract is restated from open3d's source: parity unpinned (no open3d here).
 * out_vertices / out_normals: room for the upper bound, (nv + 3 nf, 3) double; rows [0, nv + *n_new) are written.  out_normals may
 * be NULL when normals is.  out_triangles (4 nf, 3) int64.  n_new: one int of device memory that receives the number of new vertices
 * (distinct edges), or -(error bits) when the pass failed: bit 1 = a triangle index outside [0, nv), bit 2 = a probe sequence of the
 * edge table ran out (every loop on the device is bounded).  After a failure the outputs are unspecified.  The result does not depend
 * on how the threads are scheduled.  workspace: at least tgn_subdivide_midpoint_workspace_bytes(nf) bytes of device memory
 * (12 bytes per slot of a table of the next power of two >= 6 nf, + 24 nf); that function returns 0 for an unsupported nf.
 * nv + 3 nf >= 2^31 is TGN_ERR_UNSUPPORTED; negative counts and NULL pointers are TGN_ERR_INVALID_ARGUMENT (the vertex arrays may be NULL
 * when nv = 0, the triangle arrays when nf = 0: then nothing is read or written through them); both before any HIP call.
 */
size_t tgn_subdivide_midpoint_workspace_bytes(long long nf);
int tgn_subdivide_midpoint(long long nv, long long nf, const double *vertices, const double *normals, const long long *triangles,
                           double *out_vertices, double *out_normals, long long *out_triangles, int *n_new, void *workspace,
                           size_t workspace_bytes, tgn_stream_t stream);
/*
 * One scan of the preprocess loop in one call that never holds the interpreter lock (preprocess_data.py:37-52): reads the
 * ground-truth json ({"jaw": "upper"|"lower", "labels": [FDI numbers]}), remaps the labels to 0..16 (:39-44), reads the OBJ
 * with tgn_obj_read's semantics, computes the vertex normals, centres the vertices and maps [y_min, y_max] to [-1, 1]
 * (:48-50, with numpy's summation order), and holds the (n, 7) float64 rows [x y z nx ny nz label] behind *handle.
 * jaw receives the json's "jaw" string (NUL-terminated, at most jaw_cap - 1 bytes).
 * The json reader takes a top-level object whose "labels" member is an array of plain integers of at most 18 digits and whose
 * "jaw" member is a string of printable ASCII without escapes; every other member is validated as json.load would read it (strings:
 * UTF-8, no raw byte below 0x20, only the JSON escapes; numbers, true / false / null, NaN / Infinity / -Infinity; nesting up to 64).
 * TGN_ERR_UNSUPPORTED: the json is not that (floats among the labels, escapes, missing keys, a byte-order mark, anything json.load
 * refuses) or the OBJ is outside tgn_obj_read's native subset -- the caller falls back to Python;
 * TGN_ERR_INVALID_ARGUMENT: what the reference raises on (unreadable file, bad OBJ token, label count != vertex count).
 */
int tgn_scan_open(const char *obj_path, const char *json_path, double y_min, double y_max, void **handle,
                  long long *n_vertices, char *jaw, int jaw_cap);
/* Copies the rows to labeled (n,7) double and, when xyz32 is not NULL, the float32 coordinates to xyz32 (n,3); frees the
 * handle (both pointers NULL: only frees). */
int tgn_scan_take(void *handle, double *labeled, float *xyz32);
/* The loader recycles its per-scan scratch (file text, vertices, faces, normals, rows: ~25 MB for a 100 000-vertex scan) through a pool of
 * at most 64 objects; this frees them (returns how many).  Safe at any time: tgn_scan_open allocates afresh when the pool is empty. */
int tgn_scan_pool_trim(void);

#ifdef __cplusplus
}
#endif
#endif /* TGN_POINTOPS_H */
