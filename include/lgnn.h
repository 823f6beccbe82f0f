/*
 * lgnn.h — C ABI of the MI355X (gfx950) lesion-graph message-passing library (liblgnn.so).
 *
 * This is the drop-in boundary for the reference's hot path: everything beneath
 * `self.model(data.x, edge_index, data.batch)` (reference src/lesion_gnn/models/gin.py:64,
 * src/lesion_gnn/models/gat.py:92), i.e. the work PyG 2.5.1 + torch_scatter + torch_sparse do for
 * GINConv / GATConv / GCNConv / global_mean_pool (reference call sites gin.py:9,23,31,33 and
 * gat.py:9,31,51,56). Each entry point names the reference interface it replaces.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer (hipMalloc / torch caching allocator) unless marked host;
 *   - `stream` is a hipStream_t passed as void*; work is enqueued asynchronously on it;
 *   - nothing is allocated inside; scratch comes from caller-provided workspaces;
 *   - return 0 (LGNN_OK) or a negative LGNN_E* code / positive hipError_t; never throws;
 *   - no host synchronisation inside any call, so every call is hipGraph-capturable;
 *   - fp32 storage, fp32 accumulate; index arrays int32 (CSR) or int64 (edge_index / batch, as
 *     PyG hands them over).
 */
#ifndef LGNN_H
#define LGNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LGNN_ABI_VERSION 40

#define LGNN_OK 0
#define LGNN_EINVAL (-22)
#define LGNN_ENOSPC (-28)
#define LGNN_EBUSY (-16) /* a grid-barrier launch cannot have all its workgroups resident */

/* tile flag arrays (tile_open) hold ceil(N/64) + LGNN_TILE_OPEN_EXTRA int32: one flag per 64-node
 * tile, the number of flagged tiles, six words the fused GCN stack kernels use as grid-barrier
 * counters for their open-tile phase (zeroed by whoever writes the flags, re-armed by the kernels),
 * then LGNN_SLOT_FLAGS partial-slot skip words at [ceil(N/64) + LGNN_SLOT_FLAG0 + b]: set by
 * lgnn_gcn_stack_bwd_s3f for a workgroup b that processed no closed tile and so wrote no partial
 * slot, read by lgnn_node_linear_bwd_tiles(..., accumulate = 2) (see there) */
#define LGNN_SLOT_FLAG0 7
#define LGNN_SLOT_FLAGS 256
#define LGNN_TILE_OPEN_EXTRA (LGNN_SLOT_FLAG0 + LGNN_SLOT_FLAGS)

/* self-loop handling of the graph build (which PyG utility the conv applies to edge_index) */
#define LGNN_LOOPS_KEEP 0      /* GINConv: edges used as given (KNN loop=True self pairs kept) */
#define LGNN_LOOPS_REMAINING 1 /* GCNConv gcn_norm: add_remaining_self_loops (one loop/node, last) */
#define LGNN_LOOPS_READD 2     /* GATConv: remove_self_loops + add_self_loops (one loop/node, last) */

/* edge weights written by the graph build */
#define LGNN_NORM_NONE 0 /* w = 1 */
#define LGNN_NORM_GCN 1  /* w_ij = deg_j^-1/2 * deg_i^-1/2, deg = in-degree incl. loop, inf -> 0 */

/* activation fused into the node-tile kernels */
#define LGNN_ACT_NONE 0
#define LGNN_ACT_ELU 1

/* upstream-gradient source of lgnn_node_linear_bwd */
#define LGNN_GRAD_DIRECT 0   /* dY[M,N] as given */
#define LGNN_GRAD_POOL 1     /* dY[i] = dP[batch[i]] (/ count for mean pooling) */
#define LGNN_GRAD_TRANSPOSE 2 /* dY[i] = tself*dS[i] + sum_{e in T(i)} tw_e dS[tidx_e] */

int lgnn_abi_version(void);
const char* lgnn_status_string(int status);

/* Process-wide path options (ABI v38; they replace round-5's LGNN_* environment reads): the
 * alternative kernels the default path was measured against, kept selectable for the tests that
 * check the pair bit for bit. lgnn_set_option returns the previous value (LGNN_EINVAL for an
 * unknown option); lgnn_get_option the current one. Not meant to change while launches that read
 * them are being recorded into a graph.
 *   LGNN_OPT_GAT_PIPE      1 (default): the row-pipelined GATConv kernels where the shape allows;
 *                          0: the per-row kernels
 *   LGNN_OPT_GAT_BPC       0 (default): the pipelined grids are occupancy-sized; n > 0: n
 *                          workgroups per CU
 *   LGNN_OPT_GRAPH_SORTED  1 (default): the graph build tries its target-sorted path; 0: the
 *                          general counting sort always */
#define LGNN_OPT_GAT_PIPE 0
#define LGNN_OPT_GAT_BPC 1
#define LGNN_OPT_GRAPH_SORTED 2
#define LGNN_OPT_COUNT 3
int lgnn_set_option(int option, int value);
int lgnn_get_option(int option);

/* ---------------------------------------------------------------------------------------------
 * Graph structure.
 * Replaces: PyG gcn_norm / add_remaining_self_loops (GCNConv), remove_self_loops+add_self_loops
 * (GATConv, reference gat.py:31), torch_sparse ToSparseTensor CSR (reference
 * datasets/datamodule.py:44-45) — i.e. the per-forward edge_index preprocessing.
 *
 * Builds, from edge_index int64 [2, E] (row 0 = source j, row 1 = target i, any order), a CSR
 * grouped by TARGET (rowptr[N+1], col[cap] = source, w[cap]) and optionally its transpose grouped
 * by SOURCE (tptr[N+1], tidx[cap] = target, tw[cap]), cap = E + N. Within a row entries keep
 * edge_index order; with LOOPS_REMAINING / LOOPS_READD the node's single self loop is last (as
 * PyG appends loops after the edge list). Invalid indices (<0 or >= N) are dropped and counted in
 * *err_count (device int, may be NULL). tmap (nullable, needs the transpose) [cap]: for each
 * transpose entry, the position of the same edge in the target CSR (GAT backward reads per-edge
 * attention saved in target order). tile_open (nullable) [ceil(N/64) + LGNN_TILE_OPEN_EXTRA]: as lgnn_tile_open,
 * in the same launches. gptr (nullable) [num_graphs + 1]: as lgnn_batch_ptr from batch [N],
 * in the same launches. *err_count is written (not accumulated). Workspace size:
 * lgnn_graph_workspace_bytes. N + E < 2^30. Five launches, no host synchronisation.
 *
 * Target-sorted fast path (builds without the source CSR, or lazy ones; no tmap): the first
 * launch checks edge_index on the device — targets non-decreasing, indices valid, at most one
 * self loop per row, at most 16 CSR entries per row, runs of at most 64 rows without entries and
 * (lazy) no edge leaving its 64-node tile. When every check passes (k-NN input collated in graph
 * order: PyG knn_graph groups the edges by target) the third launch writes the CSR by a scan of
 * the row lengths and a coalesced copy, and the count / fill / finish launches return at once;
 * otherwise the general counting-sort launches run. Same outputs either way (bit-identical).
 * lgnn_set_option(LGNN_OPT_GRAPH_SORTED, 0) disables the fast path (A/B, tests).
 * ------------------------------------------------------------------------------------------- */
size_t lgnn_graph_workspace_bytes(int64_t num_nodes, int64_t num_edges);
int lgnn_graph_build(const int64_t* edge_index, int64_t num_edges, int64_t num_nodes, int loops,
                     int norm, int32_t* rowptr, int32_t* col, float* w, int32_t* tptr,
                     int32_t* tidx, float* tw, int32_t* tmap, int32_t* tile_open,
                     const int64_t* batch, int64_t num_graphs, int32_t* gptr, int32_t* err_count,
                     void* workspace, size_t workspace_bytes, void* stream);
/* lgnn_graph_build for a consumer that reads the source (transpose) CSR only for open tiles
 * (the fused GCN stack): tile_open and tptr required, tmap NULL; the tiles' open flags are set
 * by the count and scan passes, and tptr / tidx / tw are meaningful only when some tile is open
 * (the sorted fast path leaves them unwritten: it is taken only when no tile is open). Same target
 * CSR, flags and weights as lgnn_graph_build. */
int lgnn_graph_build_lazy(const int64_t* edge_index, int64_t E, int64_t N, int loops, int norm,
                          int32_t* rowptr, int32_t* col, float* w, int32_t* tptr, int32_t* tidx,
                          float* tw, int32_t* tmap, int32_t* tile_open, const int64_t* batch,
                          int64_t num_graphs, int32_t* gptr, int32_t* err_count, void* workspace,
                          size_t workspace_bytes, void* stream);
/* lgnn_graph_build[_lazy] (lazy != 0: the lazy variant) whose first launch also writes the split-3
 * weight planes of `job` (what lgnn_weight_planes(job->nl, job->W, job->widths, job->planes,
 * job->planes_t) writes, bitwise) as extra workgroups: the planes a fused GCN stack forward reads
 * are made from the live weights by every forward that builds its graph, with no launch of their
 * own (a captured step replays the split, so weights written between replays are seen).
 *
 * Fold slot: with LGNN_PLANE_JOB_FOLD OR-ed into nl (layers = nl without the flag, 2 <= layers <=
 * LGNN_PLANE_JOB_MAX - 1) W[layers] points to b_0 [widths[1]], in_proj's bias, and the job also
 * writes, behind the layers' slots of `planes`, one more slot: the planes of W_10 = W_1 W_0
 * ([widths[2]][widths[0]], fp32 fmaf sums over j ascending: the same bits whichever launch runs the
 * job) and behind it 128 floats b_10 = W_1 b_0 (zero past widths[2]) — in_proj folded into conv 1,
 * read by lgnn_gcn_stack_fwd_s3(_all) with has_in_proj = LGNN_S3_FWD_FOLD / _FOLD_H0. `planes` then
 * holds lgnn_weight_planes_bytes(nl) bytes with the flag in nl; planes_t is as without it. */
#define LGNN_PLANE_JOB_MAX 8
#define LGNN_PLANE_JOB_FOLD 256
typedef struct lgnn_plane_job {
  int nl;                                /* layers, 1..LGNN_PLANE_JOB_MAX */
  int widths[LGNN_PLANE_JOB_MAX + 1];    /* W[l] is [widths[l+1]][widths[l]] */
  const float* W[LGNN_PLANE_JOB_MAX];
  uint16_t* planes;                      /* lgnn_weight_planes_bytes(nl) */
  uint16_t* planes_t;                    /* nullable: the transposed planes */
} lgnn_plane_job;
int lgnn_graph_build_planes(const int64_t* edge_index, int64_t E, int64_t N, int loops, int norm,
                            int32_t* rowptr, int32_t* col, float* w, int32_t* tptr,
                            int32_t* tidx, float* tw, int32_t* tmap, int32_t* tile_open,
                            const int64_t* batch, int64_t num_graphs, int32_t* gptr,
                            int32_t* err_count, void* workspace, size_t workspace_bytes, int lazy,
                            const lgnn_plane_job* job, void* stream);

/* Diagnostic (synchronises `stream`): 1 when the last lgnn_graph_build[_lazy] on `workspace`
 * took the target-sorted fast path, 0 when it ran the general launches. Meaningful only after a
 * build that tried the fast path (see above). */
int lgnn_graph_build_path(const void* workspace, int64_t num_nodes, int64_t num_edges,
                          void* stream);

/* Graph offsets from a sorted PyG `batch` vector (Batch.ptr): ptr[g] = first node of graph g,
 * ptr[B] = M. Replaces the count/offset half of PyG scatter(reduce='mean') over `batch`. */
int lgnn_batch_ptr(const int64_t* batch, int64_t num_nodes, int64_t num_graphs, int32_t* ptr,
                   void* stream);

/* ---------------------------------------------------------------------------------------------
 * k-NN graph of a batch of point sets. Replaces: torch_cluster.knn_graph(pos, k, batch, loop,
 * flow='source_to_target') behind PyG's KNNGraph transform (reference configs/config.py:47
 * KNNGraph(k=6, loop=True); per graph in datasets/datamodule.py:43-48; sweep.py:105-120 k in
 * [2, 32]). pos [N][dims] fp64 (dims 2 or 3); batch [N] int64 sorted graph ids; ptr [B+1] int32
 * graph offsets (lgnn_batch_ptr). For every node q: its kk = min(k, n_g) (loop) or
 * min(k + 1, n_g) - 1 (!loop, q itself excluded) nearest nodes of its graph, ordered by (fp64
 * squared distance, index); edge_index [2][num_edges] int64 = (neighbour, q), grouped by q in node
 * order. num_edges = sum_g n_g * kk_g (the caller computes it to size edge_index). 1 <= k <= 32.
 * workspace: lgnn_knn_workspace_bytes(B) bytes. Deterministic, bit-exact vs the fp64 restatement.
 * ------------------------------------------------------------------------------------------- */
size_t lgnn_knn_workspace_bytes(int64_t num_graphs);
int lgnn_knn_graph(const double* pos, int64_t num_nodes, int dims, const int64_t* batch,
                   const int32_t* ptr, int64_t num_graphs, int k, int loop, int64_t* edge_index,
                   int64_t num_edges, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Radius graph of a batch of point sets (ABI v32). Replaces: torch_cluster.radius_graph(pos, r,
 * batch, loop, max_num_neighbors, flow='source_to_target') behind PyG's RadiusGraph transform,
 * the reference sweep's alternative to KNNGraph (src/lesion_gnn/scripts/sweep.py:113-118,
 * RadiusGraph(r=...) with PyG's defaults loop=False, max_num_neighbors=32; resolved by name in
 * transforms.py:19-23). For every node q of graph g: walk the nodes c of g in index order, taking
 * c when the fp64 squared distance |p_q - p_c|^2 < r * r, until limit = max_num_neighbors (loop)
 * or max_num_neighbors + 1 (!loop) are taken; without loop the pair (q, q) is then dropped
 * (torch_cluster 1.6.3's CUDA selection; its CPU kd-tree keeps a traversal-order subset when more
 * than `limit` are in range). edge_index [2][E] int64 = (c, q), grouped by q in node order, c
 * ascending. pos / batch / ptr as lgnn_knn_graph; workspace lgnn_radius_workspace_bytes(N).
 *   lgnn_radius_count: per-node counts and their scan into the workspace; the edge count E is the
 *                      int64 at byte offset N * 8 of the workspace (the caller reads it to size
 *                      edge_index: the one host synchronisation).
 *   lgnn_radius_graph: writes the edges (same workspace, untouched in between; num_edges = E).
 * Deterministic, bit-exact vs the fp64 restatement (oracle/pyg_ref.py radius_graph).
 * ------------------------------------------------------------------------------------------- */
size_t lgnn_radius_workspace_bytes(int64_t num_nodes);
int lgnn_radius_count(const double* pos, int64_t num_nodes, int dims, const int64_t* batch,
                      const int32_t* ptr, int64_t num_graphs, double r, int max_num_neighbors,
                      int loop, void* workspace, size_t workspace_bytes, void* stream);
int lgnn_radius_graph(const double* pos, int64_t num_nodes, int dims, const int64_t* batch,
                      const int32_t* ptr, int64_t num_graphs, double r, int max_num_neighbors,
                      int loop, int64_t* edge_index, int64_t num_edges, const void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Gaussian edge weights. Replaces lesion_gnn.transforms.GaussianDistance.__call__ (reference
 * src/lesion_gnn/transforms.py:49-58; known answers test/test_transforms.py:8-77), the
 * edge_weight producer of DRGNet's GraphConv stack (models/drgnet.py:55, :103):
 *   out[e] = exp(-|pos[row_e] - pos[col_e]|^2 / (2 sigma^2)) / sqrt(2 pi sigma^2)
 * evaluated in pos's precision (pos_f64: 0 = fp32, 1 = fp64; pos [num_nodes][dims], dims <= 16),
 * stored as fp32 (out_f64 = 0, the reference's default dtype) or fp64. edge_index [2][num_edges]
 * int64 (row, col). err [1] (device) = number of edges with an out-of-range index (their weight
 * is 0). num_edges == 0 is a no-op (the reference warns and leaves the graph unchanged).
 * ------------------------------------------------------------------------------------------- */
int lgnn_gaussian_distance(const void* pos, int pos_f64, int64_t num_nodes, int dims,
                           const int64_t* edge_index, int64_t num_edges, double sigma, void* out,
                           int out_f64, int32_t* err, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Node-tile fused aggregate + linear (+bias, +activation), forward.
 * Replaces: nn.Linear (reference gin.py:21 in_proj), GCNConv.lin + propagate + bias
 * (A_hat (X W^T) == (A_hat X) W^T), GINConv aggregate + first MLP Linear (reference gin.py:23),
 * with F.elu (gin.py:31) fused.
 *
 *   Y[M,N] = act( P(X) W^T + b ),  W [N,K] row-major (torch Linear layout), b [N] or NULL,
 *   P(X) = X                                   if rowptr == NULL,
 *   P(X)_i = sum_{e in row i} w_e X[col_e] + self_scale * X_i   otherwise (w == NULL: w_e = 1).
 *   S_out [M,K] (may be NULL): also store P(X) — the backward then streams it instead of
 *   re-aggregating (supported when K <= 128 and N <= 128, multiples of 4; else LGNN_EINVAL).
 * ------------------------------------------------------------------------------------------- */
int lgnn_node_linear_fwd(const float* X, int64_t M, int K, const int32_t* rowptr,
                         const int32_t* col, const float* w, float self_scale, const float* W,
                         const float* b, int N, int act, float* Y, float* S_out, void* stream);
/* Same, restricted to the 64-node tiles t with (tile_open[t] != 0) == want_open (tile_open from
 * lgnn_tile_open; NULL = every tile). Fast-path shapes only. Used to pair the layer-by-layer
 * kernels with lgnn_gcn_stack_fwd, which takes the tiles no edge leaves. */
int lgnn_node_linear_fwd_tiles(const float* X, int64_t M, int K, const int32_t* rowptr,
                               const int32_t* col, const float* w, float self_scale,
                               const float* W, const float* b, int N, int act, float* Y,
                               float* S_out, const int32_t* tile_open, int want_open,
                               void* stream);

/* ---------------------------------------------------------------------------------------------
 * Node-tile fused backward of lgnn_node_linear_fwd.
 * Replaces: autograd of nn.Linear / GCNConv / GINConv-first-Linear + F.elu + the scatter-add
 * backward (index_select / index_add_) and the global_mean_pool backward (reference gin.py:33).
 *
 *   G   = upstream gradient by grad_mode (LGNN_GRAD_*):
 *           DIRECT: dY[M,N];  POOL: dY[batch_i] (dY is [B,N]; mean: / (ptr[g+1]-ptr[g]));
 *           TRANSPOSE: tself*dY[i] + sum_{e in tptr row i} tw_e dY[tidx_e] (tw NULL: 1)
 *   dZ  = G ⊙ act'(H),  H = this layer's saved forward output [M,N] (ELU: H>0 ? 1 : H+1)
 *   dW_partial[g] (+)= dZ^T P(X) over the row tiles owned by partial slot g  ([P][N][K])
 *   db_partial[g] (+)= colsum(dZ)                                          ([P][N], may be NULL)
 *   dXpre = dZ W  [M,K]  (may be NULL)
 * The P partial slots are summed by lgnn_reduce_partials (deterministic order).
 * num_partials: lgnn_bwd_num_partials(M, N, K, rowptr != NULL) — pass that value and size the
 * slabs with it.
 * ------------------------------------------------------------------------------------------- */
int lgnn_bwd_num_partials(int64_t M, int N, int K, int gather);
int lgnn_node_linear_bwd(int grad_mode, const float* dY, const int64_t* batch, const int32_t* gptr,
                         int pool_mean, const int32_t* tptr, const int32_t* tidx, const float* tw,
                         float tself, const float* H, int act, const float* X, int64_t M, int K,
                         const int32_t* rowptr, const int32_t* col, const float* w,
                         float self_scale, const float* W, int N, float* dXpre,
                         float* dW_partial, float* db_partial, int num_partials, void* stream);

/* Same, restricted to the 64-node tiles t with (tile_open[t] != 0) == want_open; with
 * accumulate = 1 a workgroup that processed a tile adds its dW/db into partial slot blockIdx.x
 * (num_partials = lgnn_gcn_stack_bwd_partials, slots written by lgnn_gcn_stack_bwd) instead of
 * overwriting it, and a workgroup that processed none leaves its slot alone. accumulate = 2 (after
 * lgnn_gcn_stack_bwd_s3f, num_partials <= LGNN_SLOT_FLAGS): the same, except for slots whose skip
 * word in tile_open is set (the fused kernel wrote nothing there): those are written, with zeros
 * by a workgroup that processed no tile. accumulate = 3 / 4 (after the deferred-fold mode of
 * lgnn_gcn_stack_bwd_s3f, see there; tile_open required): db as for 1 / 2, the dW slot always
 * written (zeros by a workgroup that processed no tile). Fast path only. */
int lgnn_node_linear_bwd_tiles(int grad_mode, const float* dY, const int64_t* batch,
                               const int32_t* gptr, int pool_mean, const int32_t* tptr,
                               const int32_t* tidx, const float* tw, float tself, const float* H,
                               int act, const float* X, int64_t M, int K, const int32_t* rowptr,
                               const int32_t* col, const float* w, float self_scale,
                               const float* W, int N, float* dXpre, float* dW_partial,
                               float* db_partial, int num_partials, const int32_t* tile_open,
                               int want_open, int accumulate, void* stream);

/* out[i] = sum_{p < P} partial[p*len + i], fixed order (bitwise reproducible). */
int lgnn_reduce_partials(const float* partial, int num_partials, int64_t len, float* out,
                         void* stream);
/* The same for n <= 16 independent slabs in one launch (host arrays of n entries). */
int lgnn_reduce_partials_multi(int n, const float* const* partials, const int* num_partials,
                               const int64_t* len, float* const* out, void* stream);
/* lgnn_reduce_partials_multi + outer-product jobs: where factor[j] is set (factor / width may be
 * NULL for none), out_j[c * width_j + d] = sum_{p < P_j} partials_j[p * (len_j / width_j) + c] *
 * factor_j[p * width_j + d] (fixed order). One such job is out_proj's weight gradient
 * dW_out = dlogits^T pooled, queued with the stack's slab reductions. */
int lgnn_reduce_jobs(int n, const float* const* partials, const float* const* factor,
                     const int* width, const int* num_partials, const int64_t* len,
                     float* const* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sparse aggregation alone (no linear): Y_i = self_scale*X_i + sum_{e in row i} w_e X[col_e].
 * Replaces: torch_sparse spmm(adj_t, x, 'sum') / PyG propagate(aggr='add') (GINConv, and the
 * transposed pass of every conv backward when called with the transpose CSR).
 * ------------------------------------------------------------------------------------------- */
int lgnn_spmm(const int32_t* rowptr, const int32_t* col, const float* w, float self_scale,
              const float* X, int64_t M, int D, float* Y, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Readout: per-graph segmented pool fused with the out_proj Linear.
 * Replaces: global_mean_pool / global_add_pool (reference gin.py:33, gat.py:56) + out_proj
 * (gin.py:25, gat.py:46).
 *   pooled[B,D] = sum_{i in graph g} H_i (/ count if mean; empty graph -> 0)
 *   logits[B,C] = pooled Wout^T + bout        (Wout may be NULL: pool only, logits unused)
 * ------------------------------------------------------------------------------------------- */
int lgnn_pool_head_fwd(const float* H, const int32_t* gptr, int64_t B, int D, int pool_mean,
                       const float* Wout, const float* bout, int C, float* pooled,
                       float* logits, void* stream);

/* Backward of lgnn_pool_head_fwd's Linear part:
 *   dpooled = dlogits Wout;  dWout = dlogits^T pooled;  dbout = colsum(dlogits). */
int lgnn_pool_head_bwd(const float* dlogits, const float* pooled, int64_t B, int D,
                       const float* Wout, int C, float* dpooled, float* dWout, float* dbout,
                       void* stream);

/* Backward of a bare segmented pool: dH_i = dpooled[batch_i] (/ count if mean). */
int lgnn_pool_bwd(const float* dpooled, const int64_t* batch, const int32_t* gptr, int64_t M,
                  int D, int pool_mean, float* dH, void* stream);

/* ---------------------------------------------------------------------------------------------
 * BatchNorm1d + ELU (+ dropout mask) of the GIN MLP.
 * Replaces: PyG MLP([d1,d2,d2], act="ELU", norm="batch_norm") internals (reference gin.py:23):
 * torch.nn.BatchNorm1d forward/backward (training: batch statistics, running stats updated with
 * momentum and the unbiased variance; eval: running statistics), F.elu, F.dropout.
 * Statistics in fp64, deterministic. `sums` is [2N] fp64: forward (sum z, sum z^2); backward
 * (sum g, sum g*xhat) — caller-visible so a SyncBN all-reduce can run in between.
 * mask (nullable): dropout keep-mask already scaled by 1/(1-p), [M,N].
 * ------------------------------------------------------------------------------------------- */
size_t lgnn_bn_workspace_bytes(int64_t num_rows, int N);
int lgnn_bn_stats(const float* Z, int64_t M, int N, double* sums, void* workspace,
                  size_t workspace_bytes, void* stream);
/* mean/invstd/scale/shift [N] out; scale = gamma*invstd, shift = beta - mean*scale. training=0
 * reads running_mean/var; training=1 updates them (if non-NULL) and num_batches_tracked. */
int lgnn_bn_finalize(const double* sums, double count, const float* gamma, const float* beta,
                     float eps, float momentum, int training, int N, float* running_mean,
                     float* running_var, int64_t* num_batches_tracked, float* mean,
                     float* invstd, float* scale, float* shift, void* stream);
/* A = ELU(Z*scale + shift) [* mask] */
int lgnn_bn_act(const float* Z, int64_t M, int N, const float* scale, const float* shift,
                const float* mask, float* A, void* stream);
/* sums = (sum g, sum g*xhat), g = dA * mask * ELU'(Z*scale+shift), xhat = (Z-mean)*invstd */
int lgnn_bn_bwd_stats(const float* dA, const float* Z, const float* mask, int64_t M, int N,
                      const float* scale, const float* shift, const float* mean,
                      const float* invstd, double* sums, void* workspace, size_t workspace_bytes,
                      void* stream);
/* dZ = scale*(g - sum g/count - xhat * sum(g xhat)/count) (training) | scale*g (eval);
 * dgamma = sum g*xhat, dbeta = sum g (each nullable) */
int lgnn_bn_bwd_apply(const float* dA, const float* Z, const float* mask, int64_t M, int N,
                      const float* scale, const float* shift, const float* mean,
                      const float* invstd, const double* sums, double count, int training,
                      float* dZ, float* dgamma, float* dbeta, void* stream);
/* sums[2N] = the fixed-order sum of num_partials fp64 partial rows part[p][2N] (the BN-fused
 * linear kernels below write one row per workgroup); dgamma = sums[N..2N), dbeta = sums[0..N)
 * (each nullable: the backward's affine gradients, as lgnn_bn_bwd_apply's). */
int lgnn_bn_partials_reduce(const double* part, int num_partials, int N, double* sums,
                            float* dgamma, float* dbeta, void* stream);
/* lgnn_bn_partials_reduce + lgnn_bn_finalize (training) in one launch (no SyncBN all-reduce
 * between them). */
int lgnn_bn_partials_finalize(const double* part, int num_partials, int N, double* sums,
                              double count, const float* gamma, const float* beta, float eps,
                              float momentum, float* running_mean, float* running_var,
                              int64_t* num_batches_tracked, float* mean, float* invstd,
                              float* scale, float* shift, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The GIN MLP's linear layers with BatchNorm folded into them (the same arithmetic as the
 * lgnn_bn_* kernels above, without their passes over HBM). Fast-path shapes only (K, N <= 128,
 * multiples of 4); one partial row per workgroup, lgnn_bn_fused_partials(M) rows.
 * lgnn_node_linear_fwd_bn = lgnn_node_linear_fwd (no tile selection) with exactly one of
 *   stats_part: [P][2N] fp64 per-workgroup (sum y, sum y^2) of the output Y (then
 *     lgnn_bn_partials_reduce -> lgnn_bn_finalize), or
 *   bn_scale / bn_shift [K] (+ bn_mask [M,K], nullable): the input rows are first mapped to
 *     ELU(X*scale + shift) [* mask] — lgnn_bn_act fused into the load — and that activation is
 *     also written to bn_out [M,K] (the backward's dW input); no gather.
 * lgnn_node_linear_bwd_bn = lgnn_node_linear_bwd in LGNN_GRAD_DIRECT mode (no gather) with
 *   bn_mode LGNN_BN_GSTATS: the dX output is the gradient dA of a BN + ELU (+ mask) output whose
 *     input is bn_Z [M,K]; gstats_part [P][2K] receives per-workgroup (sum g, sum g*xhat)
 *     (lgnn_bn_bwd_stats fused into the dX epilogue), or
 *   bn_mode LGNN_BN_GIN (act NONE): dY is such a dA [M,N] of BN input bn_Z [M,N]; the kernel
 *     applies the BN backward (lgnn_bn_bwd_apply's dZ, with bn_sums / count / training) before
 *     using it, so dZ never goes to HBM.
 * ------------------------------------------------------------------------------------------- */
#define LGNN_BN_GSTATS 3
#define LGNN_BN_GIN 4
/* lgnn_node_linear_bwd_bn with the layer's output gradient taken from the pooled readout
 * (LGNN_GRAD_POOL, bn_mode LGNN_BN_GSTATS only): row i's gradient is
 *   (dlogits[batch[i]] . Wout)[n] (/ |graph| when pool_mean),
 * i.e. the global pool + out_proj backward (lgnn_pool_head_bwd's dpooled and lgnn_pool_bwd)
 * folded into the load, in the same arithmetic; dY is unused (NULL). The GIN model's last conv. */
int lgnn_node_linear_bwd_bn_pool(int bn_mode, const float* dY, const float* H, int act,
                                 const float* X, int64_t M, int K, const float* W, int N,
                                 float* dXpre, float* dW_partial, float* db_partial,
                                 int num_partials, const float* bn_Z, const float* bn_mask,
                                 const float* bn_scale, const float* bn_shift,
                                 const float* bn_mean, const float* bn_invstd,
                                 double* gstats_part, const double* bn_sums, double count,
                                 int training, const int64_t* batch, const int32_t* gptr,
                                 int pool_mean, const float* dlogits, const float* Wout,
                                 int num_classes, void* stream);
/* lgnn_node_linear_bwd_bn (bn_mode LGNN_BN_GSTATS) with the output gradient gathered through the
 * transpose CSR as it is loaded (ABI v21): row i's gradient is
 *   tself * dS[i] + sum_{e in T(i)} tw_e dS[tidx_e]   (LGNN_GRAD_TRANSPOSE),
 * dS [M,N] being the NEXT GINConv's pre-aggregation input gradient (its Lin1 dX). This is the
 * backward of that conv's aggregation (PyG GINConv propagate + (1 + eps) x, reference gin.py:23)
 * folded into this conv's Lin2 backward, so the aggregated gradient never goes to HBM. */
int lgnn_node_linear_bwd_bn_gather(const float* dS, const int32_t* tptr, const int32_t* tidx,
                                   const float* tw, float tself, const float* H, int act,
                                   const float* X, int64_t M, int K, const float* W, int N,
                                   float* dXpre, float* dW_partial, float* db_partial,
                                   int num_partials, const float* bn_Z, const float* bn_mask,
                                   const float* bn_scale, const float* bn_shift,
                                   const float* bn_mean, const float* bn_invstd,
                                   double* gstats_part, void* stream);
int lgnn_bn_fused_partials(int64_t num_rows);
int lgnn_node_linear_fwd_bn(const float* X, int64_t M, int K, const int32_t* rowptr,
                            const int32_t* col, const float* w, float self_scale, const float* W,
                            const float* b, int N, int act, float* Y, float* S_out,
                            double* stats_part, const float* bn_scale, const float* bn_shift,
                            const float* bn_mask, float* bn_out, void* stream);
int lgnn_node_linear_bwd_bn(int bn_mode, const float* dY, const float* H, int act,
                            const float* X, int64_t M, int K, const float* W, int N,
                            float* dXpre, float* dW_partial, float* db_partial, int num_partials,
                            const float* bn_Z, const float* bn_mask, const float* bn_scale,
                            const float* bn_shift, const float* bn_mean, const float* bn_invstd,
                            double* gstats_part, const double* bn_sums, double count,
                            int training, void* stream);

/* ---------------------------------------------------------------------------------------------
 * GATConv attention (PyG 2.5.1 GATConv(d1, d2//H, heads=H, dropout=p), reference gat.py:31:
 * concat=True, negative_slope, add_self_loops=True, bias=True) + the model's F.elu (gat.py:51).
 * XP = lin(x) [M, H*C] (lgnn_node_linear_fwd without bias). Graph: the LGNN_LOOPS_READD CSR
 * (remove_self_loops + add_self_loops). Per-edge arrays are [cap, H] in target-CSR order.
 * Shapes: C a power of two in [4, 512], H*C <= 512. edge_mask (nullable): attention dropout keep-mask
 * already scaled by 1/(1-p).
 * ------------------------------------------------------------------------------------------- */
/* a_s[i,h] = <XP[i,h,:], att_src[h,:]>, a_d likewise with att_dst (the alpha_src/alpha_dst sums) */
int lgnn_gat_att(const float* XP, int64_t M, int H, int C, const float* att_src,
                 const float* att_dst, float* a_s, float* a_d, void* stream);
/* alpha = softmax_i(leaky_relu(a_s[j] + a_d[i])) (PyG utils.softmax, +1e-16; written if
 * non-NULL), Y_i = act(sum_j alpha_ij mask_ij XP_j + bias); Y_bf16 (nullable) also receives Y
 * rounded to bf16 (RNE, torch's .to(bfloat16)): the next layer's bf16 GEMM operand */
int lgnn_gat_fwd(const int32_t* rowptr, const int32_t* col, const float* XP, const float* a_s,
                 const float* a_d, int64_t M, int H, int C, float negative_slope,
                 const float* edge_mask, const float* bias, int act, float* alpha, float* Y,
                 uint16_t* Y_bf16, void* stream);
/* Backward, target rows: dZ = dY * act'(Y); da_e = d(logit) per edge; da_d = row sums. */
int lgnn_gat_bwd_edge(const int32_t* rowptr, const int32_t* col, const float* XP,
                      const float* a_s, const float* a_d, const float* alpha,
                      const float* edge_mask, const float* dY, const float* Y, int act, int64_t M,
                      int H, int C, float negative_slope, float* dZ, float* da_e, float* da_d,
                      void* stream);
/* lgnn_gat_bwd_edge with the output gradient formed from the readout's gradient (ABI v22):
 * dY[i] = (dlogits[batch[i]] . Wout) (/ |graph| when pool_mean), with lgnn_pool_head_bwd's and
 * lgnn_pool_bwd's arithmetic (bitwise), so the GAT model's last conv needs no dH tensor: the
 * global_mean_pool / global_add_pool + out_proj backward (reference gat.py:56-58) folded into
 * this kernel's load. Wout [num_classes][H*C]; dY is not an argument. */
int lgnn_gat_bwd_edge_pool(const int32_t* rowptr, const int32_t* col, const float* XP,
                           const float* a_s, const float* a_d, const float* alpha,
                           const float* edge_mask, const float* Y, int act, int64_t M, int H,
                           int C, float negative_slope, const int64_t* batch,
                           const int32_t* gptr, int pool_mean, const float* dlogits,
                           const float* Wout, int num_classes, float* dZ, float* da_e,
                           float* da_d, void* stream);
/* Backward, source rows (transpose CSR + tmap from lgnn_graph_build): dXP, and per-block column
 * partials [P][3][H*C] = (d att_src, d att_dst, d bias) for lgnn_reduce_partials. */
int lgnn_gat_bwd_num_partials(int64_t M);
int lgnn_gat_bwd_node(const int32_t* tptr, const int32_t* tidx, const int32_t* tmap,
                      const float* alpha, const float* edge_mask, const float* da_e,
                      const float* da_d, const float* dZ, const float* XP, const float* att_src,
                      const float* att_dst, int64_t M, int H, int C, float* dXP,
                      float* partials, int num_partials, uint16_t* dXP_bf16, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused GCN layer stack, forward (one launch for the whole model body below the readout).
 * Replaces: in_proj nn.Linear (reference gin.py:21 skeleton) + L x (GCNConv + F.elu) — the
 * layer-by-layer lgnn_node_linear_fwd chain — keeping each 64-node tile on chip across layers.
 *   has_in_proj=1: H[0] = X W[0]^T + b[0] (X [M, d_in]); else layer 1 reads X (widths[0]=d_in)
 *   for l = 1..L: H[l] = ELU(Â (H[l-1] W[l]^T) + b[l]) (CSR rowptr/col/w, self loops in the
 *   CSR; PyG 2.5.1 GCNConv order: lin, then propagate, then bias).  W, b, H: host arrays of
 *   L+1 device pointers; widths[l] = output width of layer l. All widths and d_in <= 128,
 *   multiples of 4; L + 1 <= 8.
 *   tile_open (required when L >= 1): only tiles with tile_open[t] == 0 are computed — their
 *   CSR entries stay inside the tile and number at most 2048 (lgnn_graph_build /
 *   lgnn_tile_open flags); run the others with lgnn_node_linear_fwd_tiles(..., tile_open, 1).
 * ------------------------------------------------------------------------------------------- */
int lgnn_gcn_stack_fwd(const float* X, int64_t M, int d_in, int has_in_proj,
                       const int32_t* rowptr, const int32_t* col, const float* w, int L,
                       const float* const* W, const float* const* b, const int* widths,
                       float* const* H, const int32_t* tile_open, void* stream);
/* Split-3 variant of lgnn_gcn_stack_fwd: the same math and arguments, the GEMMs on bf16 MFMA at
 * fp32 accuracy — every operand held as three bf16 planes (x = hi + mid + lo to 2^-24) and each
 * product taken as the six plane products that matter (liblgnn stack3.hip). `planes` holds the
 * weights of layers 0..L as written by lgnn_weight_planes (in place of W). L >= 1.
 * adjt (nullable): ceil(M/64) * LGNN_S3_ADJT_TILE_BYTES bytes; receives, for every closed tile,
 * the tile's dense fp32 Â (64 x 64, as summed from the CSR block), which
 * lgnn_gcn_stack_bwd_s3f(_all) then loads instead of rebuilding it (same graph, same tile_open).
 * has_in_proj here (and in lgnn_gcn_stack_fwd_s3_all) selects how the closed tiles run; any other
 * value is LGNN_EINVAL:
 *   0, 1                  as lgnn_gcn_stack_fwd: without / with in_proj as a GEMM of its own
 *   LGNN_S3_FWD_FOLD      in_proj folded into conv 1 (exact: no activation between them):
 *                         H_1 = ELU(Â (X W_10^T + 1 b_10^T) + b_1) from the fold slot of `planes`
 *                         (a plane job with LGNN_PLANE_JOB_FOLD, L + 1 <= LGNN_PLANE_JOB_MAX - 1);
 *                         H[0] rows of closed tiles are NOT written (open tiles' rows are). For a
 *                         backward that does not read H_0 (lgnn_gcn_stack_bwd_s3f* with H[0] NULL).
 *   LGNN_S3_FWD_FOLD_H0   the same H_1..H_L, bit for bit, and H[0] of the closed tiles also
 *                         formed and stored as with has_in_proj = 1 (bit for bit).
 * Open tiles run in_proj and every conv on the fp32 weights in all modes: b[0], H[0] (and W[0] for
 * _all) stay required. H_1..H_L of the folded modes differ from has_in_proj = 1 at fp32 rounding
 * level (another association of the same sums). */
#define LGNN_S3_ADJT_TILE_BYTES 16384
#define LGNN_S3_FWD_FOLD 2
#define LGNN_S3_FWD_FOLD_H0 3
int lgnn_gcn_stack_fwd_s3(const float* X, int64_t M, int d_in, int has_in_proj,
                          const int32_t* rowptr, const int32_t* col, const float* w, int L,
                          const uint16_t* planes, const float* const* b, const int* widths,
                          float* const* H, const int32_t* tile_open, void* adjt, void* stream);
/* Weight planes for the split-3 kernels: nl layers, W[l] [widths[l+1], widths[l]] fp32
 * (torch Linear layout; widths <= 128, multiples of 4) -> planes[l][3][128][128] bf16 (zero
 * padded, feature order perm16), lgnn_weight_planes_bytes(nl) bytes; planes_t (nullable, same
 * size) also gets the transposed planes. One launch; rerun whenever the weights change.
 * nl may carry LGNN_PLANE_JOB_FOLD (see lgnn_plane_job): W then has layers + 1 entries, the last
 * one b_0, and `planes` also receives the fold slot and b_10 (lgnn_weight_planes_bytes(nl) with
 * the flag counts them). */
size_t lgnn_weight_planes_bytes(int nl);
int lgnn_weight_planes(int nl, const float* const* W, const int* widths, uint16_t* planes,
                       uint16_t* planes_t, void* stream);

/* Split-3 backward of the fused GCN stack for the closed tiles (tile_open[t] == 0), one launch per
 * layer (stack3_bwd.hip), the same math and outputs as lgnn_gcn_stack_bwd with any L >= 1 (L + 1 <=
 * 8): the GEMMs on bf16 MFMA at fp32 accuracy. planes_t: the transposed weight planes of layers
 * 0..L (lgnn_weight_planes(..., planes_t)); dP [num_graphs][widths[L+1]] the pooled-output
 * gradient; dz_ws: 2 * M * 128 floats of scratch (dZ between the layer launches); dWp/dbp slabs
 * with num_partials = lgnn_gcn_stack_bwd_s3_partials(M) slots, every slot written. */
int lgnn_gcn_stack_bwd_s3_partials(int64_t num_nodes);
int lgnn_gcn_stack_bwd_s3(const float* dP, const int64_t* batch, const int32_t* gptr,
                          int pool_mean, int64_t num_graphs, const int32_t* rowptr,
                          const int32_t* col, const float* w, const float* X, int64_t M, int L,
                          const uint16_t* planes_t, const float* const* H, const int* widths,
                          float* const* dWp, float* const* dbp, int num_partials, float* dz_ws,
                          const int32_t* tile_open, void* stream);
/* Tiles: 64 consecutive node rows. open[t] = 1 when an edge joins tile t to another tile (its
 * layers then depend on other tiles) or when the tile holds more than 2048 CSR entries; the
 * fused stacks skip open tiles. open has lgnn_tile_count(N) + 1 entries: the last one counts the
 * open tiles (the *_tiles kernels with want_open = 1 return at once when it is 0). */
int lgnn_tile_count(int64_t num_nodes);
int lgnn_tile_open(const int32_t* rowptr, const int32_t* col, int64_t num_nodes, int32_t* open,
                   void* stream);

/* ---------------------------------------------------------------------------------------------
 * Criterion. Replaces: nn.CrossEntropyLoss(weight=class_weights) of BaseLightningModule
 * (reference models/base.py:93-94, training_step :196-201), mean reduction.
 *   fwd: lse[B] = logsumexp(logits_i); loss[0] = sum w[y] (lse - z[y]) / sum w[y]; wsum[0] =
 *        sum w[y] (weight NULL = 1); *bad = 1 if a target is outside [0, C) (such rows skipped).
 *   bwd: dlogits = grad_loss[0] * w[y_i] / wsum * (softmax(z_i) - onehot(y_i)).
 * Deterministic (one workgroup, fixed reduction order). All pointers device pointers.
 * ------------------------------------------------------------------------------------------- */
int lgnn_ce_fwd(const float* logits, const int64_t* target, const float* weight, int64_t B, int C,
                float* lse, float* loss, float* wsum, int* bad, void* stream);
int lgnn_ce_bwd(const float* logits, const int64_t* target, const float* weight, int64_t B, int C,
                const float* lse, const float* wsum, const float* grad_loss, float* dlogits,
                void* stream);
/* lgnn_ce_fwd that also writes the logits gradient's per-row factors (ABI v35):
 * pm [B][C] = exp(z - lse) - [c == y], wt [B] = weight[y] (1 unweighted, 0 for a target outside
 * [0, C)) — lgnn_ce_src's inputs, so a consumer forms lgnn_ce_bwd's dlogits from plain loads. */
int lgnn_ce_fwd_factors(const float* logits, const int64_t* target, const float* weight,
                        int64_t B, int C, float* lse, float* loss, float* wsum, int* bad,
                        float* pm, float* wt, void* stream);
/* The CE logits gradient without materialising it (ABI v33; v35: from the readout's pm / wt): the
 * consumers form lgnn_ce_bwd's dlogits[i][c] = gloss * wt[i] / wsum * pm[i][c] themselves, bit
 * for bit (lgnn_ce_fwd_factors writes pm and wt with lgnn_ce_bwd's expressions).
 * lgnn_reduce_jobs_ce = lgnn_reduce_jobs where jobs with ce_job[j] != 0 take the [P][C] logits
 * gradient (P = B) in place of partials[j] (which may be NULL): out_proj's db (len C) and
 * dW = dlogits^T pooled (factor = pooled, len C * width). The same sums as lgnn_reduce_jobs on
 * lgnn_ce_bwd's output, bitwise. */
typedef struct lgnn_ce_src {
  const float* pm;     /* [B][C] exp(z - lse) - [c == y] (lgnn_ce_fwd_factors) */
  const float* wt;     /* [B] weight[y] (lgnn_ce_fwd_factors) */
  const float* wsum;   /* [1] */
  const float* gloss;  /* [1] gradient of the loss */
} lgnn_ce_src;
int lgnn_reduce_jobs_ce(int n, const float* const* partials, const float* const* factor,
                        const int* width, const int* num_partials, const int64_t* len,
                        float* const* out, const int* ce_job, const lgnn_ce_src* ce,
                        int num_classes, void* stream);
/* Regression head + criterion (ABI v23): pred = clamp(z, lo, hi) (reference gat.py:94-95,
 * gin.py:66-67: logits.squeeze(1).clamp(0, C - 1)) and loss = mean l(pred - y) with
 * l = nn.MSELoss (smooth_l1 = 0) or nn.SmoothL1Loss(beta = 1) (models/base.py:95-96), one
 * workgroup, fixed-order sum. target: int64 class labels (target_is_i64; the reference's
 * y.float()) or fp32 [B]. Backward: dz = [lo <= z <= hi] (grad_pred + grad_loss / B l'(pred - y));
 * grad_loss / grad_pred nullable (not both). */
int lgnn_regression_fwd(const float* z, const void* target, int target_is_i64, int64_t B,
                        float lo, float hi, int smooth_l1, float* pred, float* loss,
                        void* stream);
int lgnn_regression_bwd(const float* z, const void* target, int target_is_i64, int64_t B,
                        float lo, float hi, int smooth_l1, const float* grad_loss,
                        const float* grad_pred, float* dz, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused GCN layer stack, backward, for the tiles with tile_open[t] == 0 (L = 1 or 2 convs).
 * Replaces: the autograd chain below the readout of in_proj -> L x ELU(GCNConv) — pool broadcast
 * of dP (global_mean/add_pool backward), per conv G = Â^T dZ, dW += G^T H_{l-1}, dH = G W,
 * dZ = dH * ELU'(H) (PyG 2.5.1 GCNConv: out = propagate(lin(x)) + bias,
 * torch_geometric/nn/conv/gcn_conv.py) and dW_0 += dZ_0^T X for in_proj — with every
 * intermediate on chip.
 *   rowptr/col/w: the forward (target-row) CSR of lgnn_graph_build;
 *   W, H: host arrays of L+1 device pointers (H[l] = output of layer l, H[0] = in_proj output);
 *   widths[0..L+1] = d_in, h_0, ..., h_L; dWp/dbp: per-layer partial slabs with num_partials =
 *   lgnn_gcn_stack_bwd_partials(M) slots (reduce with lgnn_reduce_partials[_multi]).
 * Tiles with tile_open[t] != 0 are left to lgnn_node_linear_bwd_tiles(..., want_open = 1,
 * accumulate = 1) on the same slabs. No input gradient (the model input needs none).
 * ------------------------------------------------------------------------------------------- */
int lgnn_gcn_stack_bwd_partials(int64_t num_nodes);

int lgnn_gcn_stack_bwd(const float* dP, const int64_t* batch, const int32_t* gptr, int pool_mean,
                       const int32_t* rowptr, const int32_t* col, const float* w, const float* X,
                       int64_t M, int L, const float* const* W, const float* const* H,
                       const int* widths, float* const* dWp, float* const* dbp, int num_partials,
                       const int32_t* tile_open, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Optimizer step. Replaces: torch.optim.Adam / AdamW (amsgrad = False) as configured by the
 * reference (models/base.py:162-188), in one launch over up to 16 fp32 tensors.
 *   decoupled = 0: Adam (L2: g += weight_decay * p); 1: AdamW (p *= 1 - lr * weight_decay).
 *   step: device float, the number of steps taken (read by every workgroup; with advance = 1
 *   incremented once, by the last one); ticket: device uint32[9], zero before the first call
 *   (re-armed by the call). Split a longer list over several calls with advance = 0 on all but
 *   the last (every call of one step then uses the same step count).
 *   Graph-capturable (lr and the betas are launch arguments: fixed in a captured graph; for a
 *   rate that changes between replays see lgnn_adam_step_dlr).
 * ------------------------------------------------------------------------------------------- */
int lgnn_adam_step(int n, float* const* params, const float* const* grads, float* const* exp_avg,
                   float* const* exp_avg_sq, const int64_t* numels, float* step,
                   unsigned int* ticket, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int decoupled, int maximize, int advance,
                   void* stream);

/* lgnn_adam_step with the learning rate on the device: lr is a device float that every workgroup
 * reads where it reads step[0], so a write to it between two replays of a captured graph (an LR
 * scheduler's) acts on the next replay. Everything else is lgnn_adam_step's (one kernel body):
 * given the same fp32 rate the two entries give bitwise equal results. lr = NULL: LGNN_EINVAL. */
int lgnn_adam_step_dlr(int n, float* const* params, const float* const* grads,
                       float* const* exp_avg, float* const* exp_avg_sq, const int64_t* numels,
                       float* step, unsigned int* ticket, const float* lr, float beta1,
                       float beta2, float eps, float weight_decay, int decoupled, int maximize,
                       int advance, void* stream);

/* ---------------------------------------------------------------------------------------------
 * SGD step. Replaces: torch.optim.SGD as configured by the reference (models/base.py:162-188,
 * OptimizerAlgo.SGD), in one launch over up to LGNN_MAX_ADAM fp32 tensors. Per element, in
 * torch's order:
 *   g = maximize ? -grad : grad;  g += weight_decay * p
 *   momentum != 0: buf = (step == 0) ? g : momentum * buf + (1 - dampening) * g
 *                  g = nesterov ? g + momentum * buf : buf
 *   p -= lr * g
 *   momentum_buf: one buffer per tensor; NULL allowed when momentum == 0 (never read then).
 *   step / ticket: as for lgnn_adam_step (the first-step rule holds under replay); needed when
 *   momentum != 0, ignored (NULL allowed) otherwise. advance as for lgnn_adam_step.
 *   lr_dev (nullable): a device float; when given it is the rate and lr is not used.
 *   nesterov needs momentum > 0 and dampening == 0 (LGNN_EINVAL otherwise, as torch raises).
 * ------------------------------------------------------------------------------------------- */
int lgnn_sgd_step(int n, float* const* params, const float* const* grads,
                  float* const* momentum_buf, const int64_t* numels, float* step,
                  unsigned int* ticket, float lr, const float* lr_dev, float momentum,
                  float dampening, float weight_decay, int nesterov, int maximize, int advance,
                  void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused GCN stack backward on split-3 bf16 MFMA (fp32 accuracy), every layer of a tile in one
 * pass, one launch. Replaces the same autograd chain as lgnn_gcn_stack_bwd (reference path:
 * global_mean/add_pool backward, per conv G = Â^T dZ, dW += G^T H, dH = G W, ELU', and in_proj
 * dW) for tiles with tile_open[t] == 0, L = 1 or 2 convs (3 through the _all / _ce entries
 * below), every width <= 128 and % 4 == 0. L <= 2: in_proj (no activation) is folded behind the
 * first conv — no dH_0 = G_1 W_1 per tile; the workgroup sums T = G_1^T X and g = colsum G_1 over
 * its tiles and writes dW_0 = W_1^T T, db_0 = W_1^T g (the same sums in another order).
 *   planes_t: the transposed weight planes of lgnn_weight_planes (all L + 1 layers);
 *   H[0..L]: layer outputs (H[0] = in_proj output); X: model input; widths[0..L+1];
 *   dWp / dbp: per-layer partial slabs with num_partials = lgnn_gcn_stack_bwd_partials(M)
 *   slots. A workgroup that processed no closed tile writes NO slot: it sets its skip word
 *   tile_open[ceil(M/64) + LGNN_SLOT_FLAG0 + b] instead (so tile_open is written by this call,
 *   beside the barrier words), and the open tiles must then be accumulated by
 *   lgnn_node_linear_bwd_tiles(..., accumulate = 2), which writes the skipped slots (zeros where
 *   it has no tile either). accumulate = 1 after this call would add to uninitialised slots.
 *   adjt (nullable): the tile adjacencies the split-3 forward wrote for this graph (its adjt);
 *   each tile's goes straight into LDS (prefetched during the previous tile) instead of being
 *   rebuilt from the CSR.
 * ------------------------------------------------------------------------------------------- */
int lgnn_gcn_stack_bwd_s3f(const float* dP, const int64_t* batch, const int32_t* gptr,
                           int pool_mean, int64_t num_graphs, const int32_t* rowptr,
                           const int32_t* col, const float* w, const float* X, int64_t M, int L,
                           const uint16_t* planes_t, const float* const* H, const int* widths,
                           float* const* dWp, float* const* dbp, int num_partials,
                           const int32_t* tile_open, const void* adjt, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The fused GCN stack with its open-tile phase in the same launch (no separate layer-by-layer
 * launches). Tiles flagged open (an edge leaves them, or > 2048 CSR entries) share no edge with
 * closed tiles, so after the closed tiles the kernel runs them layer by layer in fp32 (the bodies
 * of lgnn_node_linear_fwd_tiles / _bwd_tiles) with a grid barrier between layers; with no open
 * tile (the count word of tile_open is 0) that phase is skipped. tile_open: the graph build's
 * [ceil(M/64) + LGNN_TILE_OPEN_EXTRA] array (its barrier words are used and re-armed).
 * lgnn_gcn_stack_fwd_s3_all = lgnn_gcn_stack_fwd_s3 + W (fp32 weights, host array of L + 1
 *   device pointers) + S (host array of L pointers: S[l - 1] [M][K_l] receives Â H_{l-1} of the
 *   open tiles, read by the backward's open phase).
 * lgnn_gcn_stack_bwd_s3f_all = lgnn_gcn_stack_bwd_s3f + the transpose CSR (tptr / tidx / tw),
 *   W, S (as above) and dS_ws (2 * M * 128 floats of workspace). L = 3 (ABI v39; this entry and
 *   _ce only): dS_ws holds 3 * M * 128 floats, its last block receives dZ_0 [M][widths[1]] (the
 *   in_proj output gradient, every row) and dWp[0] / dbp[0] are not written — the caller forms
 *   dW_0 = dZ_0^T X and db_0 = colsum dZ_0 (lgnn_s3_wgrad). With dlogits [B][C] and Wout
 *   [C][N_L] (C <= 8) the pooled-output gradient dP = dlogits Wout (out_proj backward) is formed
 *   inside the kernel and dP may be NULL (lgnn_pool_head_bwd then only needs dWout / dbout, and
 *   can run concurrently).
 * Both _all entries return LGNN_EBUSY (nothing launched) when the device cannot hold every
 * workgroup of the launch at once (its grid barriers need co-residency): the caller then runs the
 * open tiles in separate launches. lgnn_fused_grid_capacity(which) = workgroups resident at once
 * (occupancy per CU x CUs; which 0 = forward, the smallest over its has_in_proj variants — the
 * launch checks the variant it runs —, 1 = backward), or an error code (< 0). A barrier
 * that still times out (~0.5 s) counts itself in the third barrier word (tile_open[ntiles + 3]
 * forward, [ntiles + 6] backward), which stays set until the next graph build zeroes it.
 * ------------------------------------------------------------------------------------------- */
int lgnn_fused_grid_capacity(int which);
int lgnn_gcn_stack_fwd_s3_all(const float* X, int64_t M, int d_in, int has_in_proj,
                              const int32_t* rowptr, const int32_t* col, const float* w, int L,
                              const uint16_t* planes, const float* const* W,
                              const float* const* b, const int* widths, float* const* H,
                              float* const* S, int32_t* tile_open, void* adjt, void* stream);
int lgnn_gcn_stack_bwd_s3f_all(const float* dP, const int64_t* batch, const int32_t* gptr,
                               int pool_mean, int64_t num_graphs, const int32_t* rowptr,
                               const int32_t* col, const float* w, const int32_t* tptr,
                               const int32_t* tidx, const float* tw, const float* X, int64_t M,
                               int L, const uint16_t* planes_t, const float* const* W,
                               const float* const* H, const float* const* S, const int* widths,
                               float* const* dWp, float* const* dbp, int num_partials,
                               float* dS_ws, int32_t* tile_open, const float* dlogits,
                               const float* Wout, int num_classes, const void* adjt,
                               void* stream);
/* lgnn_gcn_stack_bwd_s3f_all with the logits gradient formed in the kernel from the CE forward
 * (ABI v33: lgnn_ce_src, declared with lgnn_ce_fwd below): the model + criterion backward without
 * a dlogits tensor or the lgnn_ce_bwd launch (reference models/base.py:93-94 + :196-201). The
 * same arithmetic as lgnn_ce_bwd followed by lgnn_gcn_stack_bwd_s3f_all, bitwise. */
struct lgnn_ce_src;
int lgnn_gcn_stack_bwd_s3f_ce(const int64_t* batch, const int32_t* gptr, int pool_mean,
                              int64_t num_graphs, const int32_t* rowptr, const int32_t* col,
                              const float* w, const int32_t* tptr, const int32_t* tidx,
                              const float* tw, const float* X, int64_t M, int L,
                              const uint16_t* planes_t, const float* const* W,
                              const float* const* H, const float* const* S, const int* widths,
                              float* const* dWp, float* const* dbp, int num_partials,
                              float* dS_ws, int32_t* tile_open, const struct lgnn_ce_src* ce,
                              const float* Wout, int num_classes, const void* adjt,
                              void* stream);

/* ---------------------------------------------------------------------------------------------
 * Deferred fold: a mode of lgnn_gcn_stack_bwd_s3f / _all / _ce for L <= 2, selected by
 * H[0] == NULL (nothing reads H_0 then). dW_0 = W_1^T T, db_0 = W_1^T g and
 * dW_1 = T W_0^T + g b_0^T are all linear in T = G_1^T X ([widths[2]][widths[0]]) and
 * g = colsum G_1 ([widths[2]]), so the closed tiles form none of them: each workgroup sums T and g
 * over its tiles and writes them into slot b of dWp[L + 1] / dbp[L + 1] — the host arrays hold
 * L + 2 entries in this mode (and only in this mode is that position read). EVERY workgroup
 * writes its T / g slot (zeros without a closed tile; these slabs have no skip words).
 * dbp[L + 1] holds one more 4-byte word behind its num_partials * widths[2] floats: the launch
 * writes the number of closed tiles there (int32). When it is 0 the T / g slabs are dead, as the
 * open-only slabs are without an open tile: no workgroup writes them, their reductions take the
 * word as `live`, and lgnn_gcn_fold_wgrad (its `live`) forms nothing.
 * dWp[2..L] and dbp[1..L] with their skip words are as in the legacy mode. dWp[0], dbp[0] and
 * dWp[1] receive the open tiles' directly formed sums only, overwriting: from the open phase of
 * the _all / _ce launch (if the count word of tile_open is 0 they are not written at all), or
 * after lgnn_gcn_stack_bwd_s3f from lgnn_node_linear_bwd_tiles(..., want_open = 1) with
 * accumulate = 0 for in_proj and accumulate = 4 for the first conv (its dW slot is always
 * written, zeros without a tile; its db as for accumulate = 2; 3 likewise with db as for 1),
 * accumulate = 2 above it.
 * The caller reduces the slabs — lgnn_reduce_jobs_live skips the open-only ones when no tile is
 * open — and runs lgnn_gcn_fold_wgrad once:
 *   dW0 = W1^T T (+ dW0_open), db0 = W1^T g (+ db0_open), dW1 = T W0^T + g b0^T (+ dW1_open)
 * from the reduced T [w2][d_in] and g [w2], the fp32 W0 [w1][d_in], b0 [w1] and W1 [w2][w1];
 * the *_open totals are nullable and may be the outputs themselves (added in place). live
 * (nullable device int32): 0 = T and g count as zero and are not used (outputs = the open totals). Widths
 * <= 128 and % 4 == 0 (else LGNN_EINVAL). FMA chains in index order, one thread per output
 * element (fp32; db0's in double): no atomics, bitwise repeatable.
 * lgnn_reduce_jobs_live = lgnn_reduce_jobs_ce (ce_job nullable: no CE job) + live: a host array
 * of n nullable device int32 pointers; where *live[j] == 0 the slab of job j is not read (it may
 * be uninitialised) and out_j is zeros. Live jobs sum in lgnn_reduce_jobs' order, bitwise.
 * ------------------------------------------------------------------------------------------- */
int lgnn_gcn_fold_wgrad(const float* T, const float* g, const float* W0, const float* b0,
                        const float* W1, int d_in, int w1, int w2, const float* dW0_open,
                        const float* db0_open, const float* dW1_open, const int32_t* live,
                        float* dW0, float* db0, float* dW1, void* stream);
int lgnn_reduce_jobs_live(int n, const float* const* partials, const float* const* factor,
                          const int* width, const int* num_partials, const int64_t* len,
                          float* const* out, const int* ce_job, const struct lgnn_ce_src* ce,
                          int num_classes, const int32_t* const* live, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dense GEMMs at fp32 accuracy on bf16 MFMA ("split-3"), any width. Replace: the plain
 * nn.Linear shapes outside the 128-feature tile kernels — the reference's fp32 in_proj
 * nn.Linear(1025, 128) (src/lesion_gnn/models/gat.py:29; configs/config.py:52-65) and every
 * GATConv.lin / GraphConv / in_proj wider than 128 (scripts/sweep.py:126) — forward and backward,
 * i.e. the cuBLAS addmm / mm torch runs for them.
 * Every fp32 operand is held as three bf16 planes x = hi + mid + lo (each the RNE bf16 of what the
 * planes above left) and a product as the six plane products reaching 2^-24: fp32-class results
 * (error comparable to an fp32 GEMM's). planes = 1 instead rounds each operand once to bf16 (RNE)
 * and accumulates in fp32 (the bf16 GEMM mode of BASELINE config C3, any width).
 * lgnn_s3_weight_planes: the weight operand of lgnn_s3_gemm for B = W [rows][cols] (transposed 0:
 *   Y = A W^T) or B = W^T (transposed 1: Y = A W), i.e. [ceil(out/128)][planes][128][kpad(in)]
 *   bf16 in MFMA fragment order, zero-padded; lgnn_s3_weight_planes_numel(out, in, planes) its
 *   size in elements (out = B's rows, in = B's columns).
 * lgnn_s3_weight_planes_multi: n (<= LGNN_MAX_WPREP) such operands in ONE launch (job j: W[j],
 *   rows[j], cols[j], transposed[j] -> Wp[j]; planes shared) — a model's every weight operand of a
 *   step (forward B = W and backward B = W^T) at once instead of one small launch per GEMM.
 * lgnn_s3_gemm_att: lgnn_s3_gemm (planes = 3) for a GATConv.lin (N = heads * C <= 128, no bias) that also
 *   writes the attention scores a_s[m][h] = <Y[m][hC ..), att_src[h]>, a_d likewise ([M][heads],
 *   one fmaf chain over the head's C features in feature order) — replaces lgnn_gat_att's pass.
 * lgnn_s3_gemm: Y[M][N] = A[M][K] B[N][K]^T (+ bias[N]), A fp32 (split or rounded as loaded).
 *   colsum_part (nullable): [ceil(M/64)][N] per-64-row-tile column sums of Y (fixed order).
 * lgnn_s3_wgrad: partial slabs of dW[N][K] = dY^T X (dY [M][N], X [M][K] fp32, N even):
 *   partials [num_partials][N][K], num_partials = lgnn_s3_wgrad_partials(M, K, N), summed in fixed
 *   order by lgnn_reduce_partials(_multi); db_partials (nullable) [num_partials][N] the matching
 *   column sums of dY (the bias gradient).
 * ------------------------------------------------------------------------------------------- */
size_t lgnn_s3_weight_planes_numel(int out_features, int in_features, int planes);
int lgnn_s3_weight_planes(const float* W, int rows, int cols, int transposed, int planes,
                          uint16_t* Wp, void* stream);
#define LGNN_MAX_WPREP 16
int lgnn_s3_weight_planes_multi(int n, const float* const* W, const int* rows, const int* cols,
                                const int* transposed, int planes, uint16_t* const* Wp,
                                void* stream);
int lgnn_s3_gemm(const float* A, int64_t M, int K, const uint16_t* Wp, int N, int planes,
                 const float* bias, float* Y, float* colsum_part, void* stream);
int lgnn_s3_gemm_att(const float* A, int64_t M, int K, const uint16_t* Wp, int N, int planes,
                     float* Y, const float* att_src, const float* att_dst, int heads, int C,
                     float* a_s, float* a_d, void* stream);
int lgnn_s3_wgrad_partials(int64_t M, int K, int N);
int lgnn_s3_wgrad(const float* dY, int N, const float* X, int64_t M, int K, int planes,
                  float* partials, int num_partials, float* db_partials, void* stream);
/* lgnn_s3_gemm_act (ABI v37): lgnn_s3_gemm (planes = 3, no column sums) with the activation in
 * the epilogue, Y = act(A B^T + b) (LGNN_ACT_ELU = torch's F.elu, reference gin.py:31) — the wide
 * (K or N > 128) GIN / GCN linears of the reference sweep (scripts/sweep.py:126) */
int lgnn_s3_gemm_act(const float* A, int64_t M, int K, const uint16_t* Wp, int N,
                     const float* bias, int act, float* Y, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dropout. Replaces: the Bernoulli draws of torch's dropout on the hot path — nn.Dropout between
 * GIN convs (reference src/lesion_gnn/models/gin.py:27,32), the Dropout of PyG's MLP after each
 * BatchNorm + ELU (gin.py:23) and GATConv's attention dropout (gat.py:31; PyG 2.5.1
 * F.dropout(alpha, p) before the aggregation).
 * lgnn_dropout_masks: num_masks (<= LGNN_MAX_MASKS) fp32 masks in ONE launch; mask j (host arrays:
 *   out[j] device pointer, 16-B aligned, numel[j] elements, thr[j], scale[j]) holds
 *     out[j][i] = u(j, i) >= thr[j] ? scale[j] : 0,
 *     u(j, i) = mix(key + j * 0xD1B54A32D192ED03 + i * G) >> 40,  key = mix(seed ^ counter * G),
 *   mix = the splitmix64 finalizer, G = 0x9E3779B97F4A7C15, thr = (uint32)(p * 2^24) (<= 2^24),
 *   scale = fp32(1 / (1 - p)). state: device uint64[8] = [seed, counter, ticket words (zero)]; with
 *   advance != 0 the launch increments the counter when done (a captured graph draws fresh masks
 *   per replay). The masks are a pure function of (seed, counter, j, i): the CPU oracle
 *   regenerates them bit for bit (parity with dropout on).
 * lgnn_mask_mul: y = x * mask elementwise (n floats, 16-B aligned; y may alias x) — the dropout
 *   product and its backward dx = dy * mask.
 * ------------------------------------------------------------------------------------------- */
#define LGNN_MAX_MASKS 16
int lgnn_dropout_masks(int num_masks, float* const* out, const int64_t* numel,
                       const uint32_t* thr, const float* scale, uint64_t* state, int advance,
                       void* stream);
int lgnn_mask_mul(const float* x, const float* mask, float* y, int64_t n, void* stream);
/* lgnn_act_bwd (ABI v37): dZ = dY * act'(H) elementwise from the activation's saved output H
 * (act = LGNN_ACT_ELU: 1 where H > 0, H + 1 elsewhere — F.elu's autograd, reference gin.py:31);
 * n floats, 16-B aligned; dZ may alias dY */
int lgnn_act_bwd(const float* dY, const float* H, float* dZ, int64_t n, int act, void* stream);
/* lgnn_add_act: y = act(a + b) over n floats (act = LGNN_ACT_ELU): the sum of GraphConv's two
 * branches (lin_rel's aggregation and lin_root, reference drgnet.py:33-36) with the F.elu DRGNet
 * applies to it (drgnet.py:57), so that the eager and the compiled model run the same kernel
 * there. Its backward is lgnn_act_bwd from y, handed to both branches. */
int lgnn_add_act(const float* a, const float* b, float* y, int64_t n, int act, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sort pooling (DGCNN). Replaces: PyG 2.5.1 SortAggregation(k) as DRGNet applies it to the
 * concatenated GraphConv outputs (reference src/lesion_gnn/models/drgnet.py:37, called at :59).
 *   x [M, D] fp32 (rows of one graph contiguous, PyG Batch order), gptr [B+1] int32 (Batch.ptr);
 *   out [B, k*D]: per graph the rows sorted by the LAST channel descending (ties: node order,
 *   i.e. a stable sort), the first k kept, missing rows 0; fill = min(x) - 1 and every element
 *   equal to fill is 0 (PyG's masked_fill). rank [M] int32: each node's output row, or -1;
 *   fill [1]: device float, written (read by the backward). Workspace:
 *   lgnn_sort_pool_workspace_bytes(). 1 <= k <= 4096. Two launches.
 * lgnn_sort_pool_bwd: dx [M, D] = dout[batch[i], rank[i], :] where rank[i] >= 0 and
 *   x[i, d] != fill, else 0. One launch.
 * ------------------------------------------------------------------------------------------- */
size_t lgnn_sort_pool_workspace_bytes(void);
int lgnn_sort_pool_fwd(const float* x, int64_t num_nodes, int dims, const int32_t* gptr,
                       int64_t num_graphs, int k, float* out, int32_t* rank, float* fill,
                       void* workspace, size_t workspace_bytes, void* stream);
int lgnn_sort_pool_bwd(const float* dout, const float* x, const int32_t* rank,
                       const int64_t* batch, const float* fill, int64_t num_nodes, int dims,
                       int k, float* dx, void* stream);

/* ---------------------------------------------------------------------------------------------
 * DRGNet head. Replaces: the torch modules DRGNet runs after SortAggregation (reference
 * src/lesion_gnn/models/drgnet.py:38-48, called at :60-64): Conv1d(1, c0, D, stride D) -> ELU ->
 * MaxPool1d(2, 2) -> Conv1d(c0, c1, 5) -> ELU -> flatten -> Lin(dense, H) -> ELU -> dropout ->
 * Lin(H, C), i.e. MIOpen convolutions, hipBLAS linears and the elementwise launches between them.
 *   x [B, k*D] fp32, the sort-pooled rows (row r of graph b at x[b, r*D ..)); conv1_w [c0, 1, D],
 *   conv2_w [c1, c0, 5], lin0_w [H, dense], lin1_w [C, H] and their biases, as the modules hold
 *   them. K2 = k / 2 (an odd k drops its last row, as MaxPool1d does), P = K2 - 4,
 *   dense = c1 * P (anything else: LGNN_EINVAL). mask (nullable) [B, H]: the dropout mask, 0 or
 *   1 / (1 - p), applied after Lin0's ELU. logits [B, C].
 *   Saved by the forward for the backward: a1 [B, K2, c0] (pooled ELU outputs), sel
 *   [B, K2, ceil(c0 / 16)] (bit i % 16 of word i / 16: the pool took the SECOND row of the pair
 *   for channel i; a tie takes the first, as torch's max_pool1d), a2 [B, dense], h [B, H] (Lin0's
 *   ELU output before the mask).
 * Limits (else LGNN_EINVAL, before any launch): 1 <= D <= 4097, 10 <= k <= 512, 1 <= c0, c1 <= 64,
 *   1 <= H <= 256, 1 <= C <= 16, B >= 1; for the backward also (B + 64) * max(dense, H + 1) < 2^29
 *   (the weight-gradient GEMM's 32-bit offsets). One launch.
 * lgnn_drgnet_head_bwd: dx [B, k*D] (the dropped row of an odd k: exactly 0) and the eight
 *   parameter gradients from dlogits [B, C]. He = H + H % 2: dlin0_w has room for [He, dense],
 *   dlin0_b for [He] floats (the first H rows are the gradient), dh [B, He] is scratch (Lin0's
 *   pre-activation gradient). No floating-point atomics; every sum in a fixed order (bitwise
 *   reproducible). Workspace: lgnn_drgnet_head_workspace_bytes (0: unsupported shape), at most
 *   512 slabs of the small gradients and lgnn_s3_wgrad's slabs of dlin0_w, whatever B. Three
 *   launches: the per-graph kernel, lgnn_s3_wgrad, lgnn_reduce_partials_multi.
 * ------------------------------------------------------------------------------------------- */
size_t lgnn_drgnet_head_workspace_bytes(int64_t num_graphs, int k, int dims, int c0, int c1,
                                        int hidden, int classes);
int lgnn_drgnet_head_fwd(const float* x, int64_t num_graphs, int k, int dims,
                         const float* conv1_w, const float* conv1_b, int c0,
                         const float* conv2_w, const float* conv2_b, int c1, const float* lin0_w,
                         const float* lin0_b, int hidden, int dense, const float* lin1_w,
                         const float* lin1_b, int classes, const float* mask, float* logits,
                         float* a1, uint16_t* sel, float* a2, float* h, void* stream);
int lgnn_drgnet_head_bwd(const float* dlogits, const float* x, int64_t num_graphs, int k, int dims,
                         const float* conv1_w, int c0, const float* conv2_w, int c1,
                         const float* lin0_w, int hidden, int dense, const float* lin1_w,
                         int classes, const float* mask, const float* a1, const uint16_t* sel,
                         const float* a2, const float* h, float* dx, float* dh, float* dconv1_w,
                         float* dconv1_b, float* dconv2_w, float* dconv2_b, float* dlin0_w,
                         float* dlin0_b, float* dlin1_w, float* dlin1_b, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Lesion-node feature pooling. Replaces: extract_features_by_cc (reference
 * src/lesion_gnn/datasets/nodes/lesions.py:88-93, called at :172) — torch_scatter
 * scatter(features.view(C, H*W).T, cc.flatten(), 0, reduce) with reduce "mean" or "max"
 * (FeaturesReduction, lesions.py:62-64).
 *   features [C, num_pixels] fp32 channel-major (the encoder's (1, C, H, W), contiguous);
 *   cc [num_pixels] int64 component labels; out [num_segments, C] fp32 (num_segments =
 *   max(cc) + 1 as PyG sizes it): mean = sum / max(count, 1); max of an empty segment = 0.
 *   Labels outside [0, num_segments) are skipped and counted in *err (written). counts_out
 *   [num_segments] int32 (nullable): pixels per label. 1 <= num_segments <= 4032. Workspace:
 *   lgnn_cc_pool_workspace_bytes. Two launches + two memsets, no host synchronisation.
 * ------------------------------------------------------------------------------------------- */
#define LGNN_CC_POOL_MAX_SEGMENTS 4032
size_t lgnn_cc_pool_workspace_bytes(int64_t num_pixels, int channels, int num_segments);
int lgnn_cc_pool(const float* features, int channels, int64_t num_pixels, const int64_t* cc,
                 int num_segments, int reduce_max, float* out, int32_t* counts_out, int32_t* err,
                 void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Lesion nodes from a segmentation output. Replace: the argmax + adaptive max pool, the OpenCV
 * connectedComponentsWithStats call and the host round trip between them (reference
 * src/lesion_gnn/datasets/nodes/lesions.py:150-160). Images are row-major (height, width).
 * lgnn_label_pool: logits [classes, in_height, in_width] fp32, 1 <= classes <= 255 -> out
 *   [height, width] uint8 = adaptive_max_pool2d(argmax(logits, 0), (height, width)): the argmax
 *   takes the first index among equal maxima; output row i covers input rows
 *   [floor(i * in_height / height), ceil((i + 1) * in_height / height)), columns likewise (also
 *   when height > in_height). One launch; the argmax map is never stored.
 * lgnn_ccl: image [height, width] uint8, nonzero = foreground (pixels of different nonzero
 *   values that touch are one component, OpenCV's rule); connectivity 4 or 8. labels
 *   [height * width] int64: 0 for the background (also when the image has none), components
 *   numbered 1, 2, ... in raster order of their first pixel (smallest y * width + x:
 *   scipy.ndimage.label's numbering, a pure function of the image). num_labels [1] int32 on the
 *   device: components + 1. Workspace: lgnn_ccl_workspace_bytes(height, width) (0 for sizes the
 *   entry refuses). height * width < 2^31. Six launches, no host synchronisation, no workgroup
 *   waits on another.
 * lgnn_ccl_stats: labels [height * width] int64 in [0, num_labels) -> stats [num_labels, 5]
 *   int32 (left, top, width, height, area: OpenCV's columns; row 0 is the background's) and
 *   centroids [num_labels, 2] fp64 (mean x, mean y) = double(integer sum) / double(area). A
 *   label without a pixel gets zeros in both. Labels outside the range are skipped and counted
 *   in *err (written). Three launches.
 * ------------------------------------------------------------------------------------------- */
int lgnn_label_pool(const float* logits, int classes, int in_height, int in_width, uint8_t* out,
                    int height, int width, void* stream);
size_t lgnn_ccl_workspace_bytes(int height, int width);
int lgnn_ccl(const uint8_t* image, int height, int width, int connectivity, int64_t* labels,
             int32_t* num_labels, void* workspace, size_t workspace_bytes, void* stream);
int lgnn_ccl_stats(const int64_t* labels, int height, int width, int num_labels, int32_t* stats,
                   double* centroids, int32_t* err, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Lesion nodes for a batch of images of one size: the chain above and the feature pooling for
 * every image of a batch (reference lesions.py:147-176 per image; the reference takes one image
 * per call), with launch counts that do not depend on the batch size. Additions to the ABI: the
 * one-image entries above are unchanged. batch * height * width < 2^31 in all of them.
 * lgnn_label_pool_batch: logits [batch, classes, in_height, in_width] -> out [batch, height,
 *   width] uint8; per image exactly lgnn_label_pool. One launch.
 * lgnn_ccl_batch: image [batch, height, width] uint8 -> labels [batch * height * width] int64,
 *   per image exactly what lgnn_ccl gives for it alone: 0 the background, components 1, 2, ...
 *   in raster order of their first pixel, restarting in every image; no component joins two
 *   images. num_labels [batch] int32 (components + 1 per image) and node_ptr [batch + 1] int64,
 *   the exclusive scan of num_labels, on the device. Workspace:
 *   lgnn_ccl_batch_workspace_bytes (0 for sizes the entry refuses). Six launches.
 * lgnn_ccl_stats_batch: labels as above, node_ptr [batch + 1] on the device, total_nodes =
 *   node_ptr[batch] (the caller's copy) -> stats [total_nodes, 5] int32 and centroids
 *   [total_nodes, 2] fp64 as lgnn_ccl_stats gives them, row node_ptr[b] + l for label l of image
 *   b, in the image's own coordinates. Labels outside [0, node_ptr[b + 1] - node_ptr[b]) are
 *   skipped and counted in *err (written); an image whose node_ptr words leave [0, total_nodes]
 *   has every label counted there. Three launches.
 * lgnn_cc_pool_resample: features [batch, channels, src_height, src_width] fp32, labels [batch,
 *   height, width] int64, node_ptr as above -> out [total_nodes, channels] fp32: row
 *   node_ptr[b] + l is the mean (sum / max(count, 1)) or max (0 for an empty label) over the
 *   pixels of label l of image b of the source map sampled bilinearly at (height, width),
 *   align_corners = False as torch.nn.functional.interpolate: src = (src_height / height) *
 *   (i + 0.5) - 0.5 clamped at 0 (formed in double, once per row and column), taps floor(src)
 *   and the next row (clamped at the border) with the fp32 weights 1 - lambda and lambda,
 *   columns likewise, value = wy0 * (wx0 * v00 + wx1 * v01) + wy1 * (wx0 * v10 + wx1 * v11) in
 *   fp32. The sampled map is never stored. With (height, width)
 *   == (src_height, src_width) the value is the source's, bit for bit, read in place. Otherwise
 *   one source map is staged in LDS: src_height * src_width * 4 <=
 *   LGNN_CC_POOL_RESAMPLE_MAX_SOURCE_BYTES (128 x 128), else LGNN_EINVAL. max_nodes: an upper
 *   bound of the labels per image, 1 <= max_nodes <= LGNN_CC_POOL_MAX_SEGMENTS; it sizes the LDS
 *   bins (the smaller, the more workgroups a CU holds), and labels at or above it are skipped
 *   and counted in *err like those outside the image's range. counts_out [total_nodes] int32
 *   (nullable): pixels per label. No float atomics: two calls give the same bits. Workspace:
 *   lgnn_cc_pool_resample_workspace_bytes. Two launches + two memsets.
 * ------------------------------------------------------------------------------------------- */
#define LGNN_CC_POOL_RESAMPLE_MAX_SOURCE_BYTES 65536
int lgnn_label_pool_batch(const float* logits, int batch, int classes, int in_height,
                          int in_width, uint8_t* out, int height, int width, void* stream);
size_t lgnn_ccl_batch_workspace_bytes(int batch, int height, int width);
int lgnn_ccl_batch(const uint8_t* image, int batch, int height, int width, int connectivity,
                   int64_t* labels, int32_t* num_labels, int64_t* node_ptr, void* workspace,
                   size_t workspace_bytes, void* stream);
int lgnn_ccl_stats_batch(const int64_t* labels, int batch, int height, int width,
                         const int64_t* node_ptr, int total_nodes, int32_t* stats,
                         double* centroids, int32_t* err, void* stream);
size_t lgnn_cc_pool_resample_workspace_bytes(int batch, int height, int width, int total_nodes);
int lgnn_cc_pool_resample(const float* features, int batch, int channels, int src_height,
                          int src_width, const int64_t* labels, int height, int width,
                          const int64_t* node_ptr, int total_nodes, int max_nodes, int reduce_max,
                          float* out, int32_t* counts_out, int32_t* err, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * bf16 dense GEMMs (bf16 GEMM operands rounded round-to-nearest-even as torch's
 * .to(torch.bfloat16), fp32 accumulation and output). Replace the bf16 nn.Linear / GATConv.lin
 * GEMMs of the bf16 configuration — in_proj (reference src/lesion_gnn/models/gat.py:29,
 * nn.Linear(1025, 128)) and GATConv.lin (gat.py:31, PyG Linear(bias=False)) — forward and
 * backward. Weight operands: lgnn_bf16_weight_prep writes Wb = bf16 W as a zero-padded
 * [128][lgnn_bf16_kpad(K)] matrix and, when WTb != NULL (requires K <= 128), WTb = bf16 W^T as
 * [128][lgnn_bf16_kpad(N)], both in MFMA fragment order: element (r, q) at
 * ((((q / 16) * 4 + r / 32) * 64 + 32 ((q / 8) & 1) + r % 32) * 8 + q % 8.
 *   lgnn_bf16_gemm: Y[M][N] = A[M][K] W^T (+ bias), N <= 128; A fp32 (a_is_f32 = 1, rounded
 *     as loaded, any K) or bf16 (K % 4 == 0); writes Y fp32 and/or Yb bf16 (either nullable);
 *     colsum_part (nullable) [ceil(M / 64)][N]: each 64-row tile's column sums of Y (sum them
 *     with lgnn_reduce_partials: the bias gradient of a following Linear, fixed order).
 *     For dX: A = dY (bf16, K = N), Wb = WTb, N = K.
 *   lgnn_bf16_wgrad: partials [num_partials][N][K] of dW = dY^T X (dYb bf16 [M][N], N even;
 *     X fp32 or bf16 [M][K]); num_partials from lgnn_bf16_wgrad_partials(M, K); sum them with
 *     lgnn_reduce_partials (fixed order). M * K * 4 < 2^31 for both entries.
 * ------------------------------------------------------------------------------------------- */
int lgnn_bf16_kpad(int K);
int lgnn_bf16_weight_prep(const float* W, int N, int K, uint16_t* Wb, uint16_t* WTb,
                          void* stream);
/* lgnn_bf16_weight_prep for n <= 8 weights in one launch (ABI v20): W[j] [N[j]][K[j]] fp32 ->
 * Wb[j] (and WTb[j], nullable, when K[j] <= 128), the same operands as n separate calls. The
 * bf16 GAT forward prepares in_proj's and every GATConv.lin's operands this way once per step. */
int lgnn_bf16_weight_prep_multi(int n, const float* const* W, const int* N, const int* K,
                                uint16_t* const* Wb, uint16_t* const* WTb, void* stream);
int lgnn_bf16_gemm(const void* A, int a_is_f32, int64_t M, int K, const uint16_t* Wb,
                   const float* bias, int N, float* Y, uint16_t* Yb, float* colsum_part,
                   void* stream);
/* lgnn_bf16_gemm for GATConv.lin's forward with the attention scores in its epilogue (ABI v24):
 * Y = bf16(A) bf16(W)^T (A bf16, or fp32 rounded as loaded; 64 < K <= 128; no bias;
 * N = H * C <= 128) and
 * a_s[m][h] = <Y[m][hC .. hC + C), att_src[h]>, a_d likewise with att_dst (PyG GATConv
 * alpha_src / alpha_dst, reference gat.py:31), so lgnn_gat_att does not run. */
int lgnn_bf16_gemm_att(const void* A, int a_is_f32, int64_t M, int K, const uint16_t* Wb, int N,
                       float* Y, uint16_t* Yb, const float* att_src, const float* att_dst, int H,
                       int C, float* a_s, float* a_d, void* stream);
int lgnn_bf16_wgrad_partials(int64_t M, int K);
int lgnn_bf16_wgrad(const uint16_t* dYb, int N, const void* X, int x_is_f32, int64_t M, int K,
                    float* partials, int num_partials, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Evaluation: grading metrics accumulated on the device (ABI v40). Replaces: validation_step /
 * test_step / logits_to_preds of BaseLightningModule (reference models/base.py:190-233), its
 * torchmetrics collections (:120-145: multiclass Accuracy(micro), CohenKappa(quadratic), macro
 * F1Score / Precision / Recall) and the referable-DR metrics of metrics.py:7-83 (binary accuracy,
 * F1, precision, recall, AUROC, average precision of "grade >= 2").
 *
 * One evaluator's state is caller-allocated device memory, zero before the first update:
 *   counts   int64 [C*C + LGNN_EVAL_EXTRA]: the confusion matrix [target][pred], then at
 *            C*C + LGNN_EVAL_TN / _FP / _FN / _TP the referable counts, at + LGNN_EVAL_NSEEN the
 *            rows counted and at + LGNN_EVAL_NBAD the rows whose target is outside [0, C);
 *   loss_acc double [2]: the loss numerator and denominator;
 *   scores   float [capacity], positive int32 [capacity]: per counted row (in arrival order) the
 *            referable score and whether its target is referable. Probabilistic mode only.
 *
 * lgnn_eval_update: one batch, one launch (one workgroup), graph-capturable. Per row i:
 *   probabilistic (regression = 0; z [B][C] logits, weight [C] nullable): pred = the lowest index
 *     among the maxima of z_i (upward scan with a strict >, so a NaN never wins); score =
 *     sum_{c >= 2} softmax(z_i)[c] (fp32, max subtracted, classes in ascending order); referable
 *     pred = score > 0.5 (strict: torchmetrics' binary format of probabilities); loss terms
 *     w[y] (lse - z[y]) and w[y] (lgnn_ce_fwd's, fp32) summed into loss_acc in double;
 *   regression (regression = 1; z [B]): p = clamp(z_i, 0, C - 1); pred = round(p), half to even
 *     (torch.round); referable pred = pred >= 2; loss term l(p - y) (smooth_l1 as
 *     lgnn_regression_fwd) into loss_acc[0], 1 into loss_acc[1]; nothing is stored in scores;
 *   both: referable target = y >= 2; a target outside [0, C) adds 1 to n_bad and to nothing else.
 *   The counters are integers (order-independent), the loss sums run in a fixed order, and the
 *   append offset is read from the device-side n_seen: replays of a captured update append where
 *   the previous one ended, bit for bit what eager updates give. Rows past `capacity` are counted
 *   but not stored. 1 <= C <= LGNN_EVAL_MAX_CLASSES, 1 <= B < 2^31.
 *
 * lgnn_eval_compute: result [LGNN_EVAL_RESULTS] doubles, once per epoch; a memset and two launches
 * (probabilistic) or one launch (regression), no host synchronisation. From the counters, in
 * double: micro accuracy; quadratic kappa 1 - sum w O / sum w E, w = (i - j)^2, E = rows x cols
 * / n; macro F1 / precision / recall = the mean over the classes with tp + fp + fn > 0
 * (torchmetrics 1.3.1) of 2tp / (2tp + fp + fn), tp / (tp + fp), tp / (tp + fn); the referable
 * accuracy, F1, precision, recall; loss = loss_acc[0] / loss_acc[1]. Every zero denominator gives
 * 0, except kappa's (NaN, as the reference's). From the stored scores, exact AUROC and average
 * precision by pairwise counting: for each positive i, with gt_i / eq_i = the negatives j with
 * s_j < s_i / s_j == s_i and tp_i / fp_i = the positives / negatives with s_j >= s_i,
 *   AUROC = sum_i (gt_i + eq_i / 2) / (n+ n-),   AUPRC = sum_i tp_i / (tp_i + fp_i) / n+
 * (the tie-aware trapezoid and step integrals of torchmetrics' thresholds=None curves). The pair
 * counts are integers: each thread owns one sample i, the j side is streamed through LDS in
 * chunks of LGNN_EVAL_RANK_CHUNK, chunks are dealt over LGNN_EVAL_RANK_SPLIT workgroups per i
 * block, whose counts meet in per-sample integer atomics; a single workgroup then sums them in a
 * fixed order. A NaN score compares false with everything, so its sample adds nothing to either
 * sum. This library's own definition:
 * AUROC is NaN when n+ == 0 or n- == 0, AUPRC when n+ == 0, and both when the score buffer
 * overflowed (n_seen > capacity; result[LGNN_EVAL_R_OVERFLOW] = 1) or in regression mode.
 * workspace: lgnn_eval_workspace_bytes(capacity) bytes, 16-byte aligned (unused in regression
 * mode).
 *
 * lgnn_eval_merge: adds src's counters and loss sums to dst's and appends src's stored scores to
 * dst's (one launch; both states of the same C and capacity; src unchanged): what one evaluator
 * fed both streams holds. scores / positive NULL on both sides: a regression state.
 * ------------------------------------------------------------------------------------------- */
#define LGNN_EVAL_MAX_CLASSES 64
#define LGNN_EVAL_RANK_CHUNK 1024
#define LGNN_EVAL_RANK_SPLIT 16
#define LGNN_EVAL_TN 0
#define LGNN_EVAL_FP 1
#define LGNN_EVAL_FN 2
#define LGNN_EVAL_TP 3
#define LGNN_EVAL_NSEEN 4
#define LGNN_EVAL_NBAD 5
#define LGNN_EVAL_EXTRA 6
#define LGNN_EVAL_R_MICRO_ACC 0
#define LGNN_EVAL_R_KAPPA 1
#define LGNN_EVAL_R_MACRO_F1 2
#define LGNN_EVAL_R_MACRO_PRECISION 3
#define LGNN_EVAL_R_MACRO_RECALL 4
#define LGNN_EVAL_R_ACC 5
#define LGNN_EVAL_R_F1 6
#define LGNN_EVAL_R_PRECISION 7
#define LGNN_EVAL_R_RECALL 8
#define LGNN_EVAL_R_AUROC 9
#define LGNN_EVAL_R_AUPRC 10
#define LGNN_EVAL_R_LOSS 11
#define LGNN_EVAL_R_NSEEN 12
#define LGNN_EVAL_R_NBAD 13
#define LGNN_EVAL_R_OVERFLOW 14
#define LGNN_EVAL_RESULTS 16
int lgnn_eval_update(const float* z, const int64_t* target, const float* weight, int64_t B, int C,
                     int regression, int smooth_l1, int64_t* counts, double* loss_acc,
                     float* scores, int32_t* positive, int64_t capacity, void* stream);
size_t lgnn_eval_workspace_bytes(int64_t capacity);
int lgnn_eval_compute(const int64_t* counts, const double* loss_acc, const float* scores,
                      const int32_t* positive, int64_t capacity, int C, int regression,
                      double* result, void* workspace, size_t workspace_bytes, void* stream);
int lgnn_eval_merge(int C, int64_t* counts, double* loss_acc, float* scores, int32_t* positive,
                    const int64_t* src_counts, const double* src_loss_acc,
                    const float* src_scores, const int32_t* src_positive, int64_t capacity,
                    void* stream);

/* ---------------------------------------------------------------------------------------------
 * Set attention (additive to ABI v40). Replaces: the hot path of PyG 2.5.1
 * torch_geometric/nn/aggr/utils.py — MultiheadAttentionBlock (torch.nn.MultiheadAttention on
 * to_dense_batch-padded sets with a key_padding_mask, the residual Linear + ReLU and the two
 * LayerNorms), SetAttentionBlock, InducedSetAttentionBlock, PoolingByMultiheadAttention — and of
 * set_transformer.py SetTransformerAggregation, as the reference model composes them
 * (src/lesion_gnn/models/set_transformer.py:34-66). Sets are ragged: the rows of set g are the
 * contiguous range a pointer array delimits (Batch.ptr, lgnn_batch_ptr), never padded or masked.
 *
 * lgnn_set_attn_fwd: per set g and head h, out = softmax(q_h k_h^T / sqrt(D)) [* mask] v_h.
 *   q, k, v: fp32 rows with row strides ldq / ldk / ldv (in floats; head h at columns
 *   [h * D, (h + 1) * D)), so they may be column blocks of one packed projection output.
 *   Keys / values of set g: rows kptr[g] .. kptr[g + 1], or (kptr NULL) k_rows rows per set at
 *   row g * k_rows. Queries: rows qptr[g] .. qptr[g + 1]; or (qptr NULL) q_rows rows per set at
 *   row g * q_rows; or (qptr NULL, q_shared = 1) the SAME q_rows rows [0, q_rows) of q for every
 *   set (PMA's seed points, ISAB's inducing points: no per-set copy of q). out [rows][H * D]
 *   contiguous, rows as the queries' (shared: num_sets * q_rows, set g at row g * q_rows);
 *   lse [rows][H]: the log-sum-exp of each (query row, head)'s scaled scores. No score or
 *   probability matrix is written. A set without keys gives zero output rows (lse 0).
 *   mask (nullable, with mask_off): attention-probability dropout keep-mask already scaled by
 *   1 / (1 - p) (torch.nn.MultiheadAttention(dropout = p) in training: the probabilities are
 *   dropped after the softmax), laid out [set][head][query][key]: element
 *   mask[mask_off[g] + (h * nq_g + i) * nk_g + j]; mask_off int64 [num_sets + 1] from
 *   lgnn_set_attn_mask_offsets (mask_off[num_sets] = the mask's size). The mask is a span of one
 *   lgnn_dropout_masks launch.
 *   1 <= D <= LGNN_SET_ATTN_MAX_D, H * D <= LGNN_SET_ATTN_MAX_HD, else LGNN_EINVAL. Query rows
 *   are processed in blocks of LGNN_SET_ATTN_QROWS and key rows in blocks of
 *   LGNN_SET_ATTN_KROWS, in a fixed order with a running maximum and sum: any set size.
 * lgnn_set_attn_bwd: dq, dk, dv (row strides lddq / lddk / lddv, the layouts of q, k, v) from
 *   dout, with the probabilities recomputed from q, k and lse; out is the forward's output. For
 *   shared queries dq is PER SET, [num_sets * q_rows] rows (set g at row g * q_rows): the caller
 *   sums the sets in fixed order (lgnn_reduce_partials with num_partials = num_sets,
 *   len = q_rows * lddq). Every row of dq, dk, dv is written (zeros for a set without keys or
 *   without queries). No atomics: two runs agree bit for bit.
 * ------------------------------------------------------------------------------------------- */
#define LGNN_SET_ATTN_QROWS 16
#define LGNN_SET_ATTN_KROWS 32
#define LGNN_SET_ATTN_MAX_D 128
#define LGNN_SET_ATTN_MAX_HD 512
int lgnn_set_attn_mask_offsets(const int32_t* qptr, int q_rows, const int32_t* kptr, int k_rows,
                               int64_t num_sets, int heads, int64_t* mask_off, void* stream);
int lgnn_set_attn_fwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v,
                      int64_t ldv, const int32_t* qptr, int q_rows, int q_shared,
                      const int32_t* kptr, int k_rows, int64_t num_sets, int heads, int head_dim,
                      const float* mask, const int64_t* mask_off, float* out, float* lse,
                      void* stream);
int lgnn_set_attn_bwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v,
                      int64_t ldv, const int32_t* qptr, int q_rows, int q_shared,
                      const int32_t* kptr, int k_rows, int64_t num_sets, int heads, int head_dim,
                      const float* mask, const int64_t* mask_off, const float* out,
                      const float* dout, const float* lse, float* dq, int64_t lddq, float* dk,
                      int64_t lddk, float* dv, int64_t lddv, void* stream);

/* Residual + activation + LayerNorm: y = LN(a + act(b)) over rows of C <= 512 channels.
 * Replaces: MultiheadAttentionBlock's `out = out + x; out = layer_norm1(out)` and
 * `out = out + lin(out).relu(); out = layer_norm2(out)` (PyG aggr/utils.py) and PMA's
 * `lin(x).relu()` — torch.nn.LayerNorm(C) (biased variance, eps), F.relu, the adds and their
 * autograd. act: LGNN_ACT_NONE or LGNN_ACT_RELU. a: [M][C]; or (a_rows > 0) [a_rows][C] broadcast,
 * row r reading a[r % a_rows] (the shared seed / inducing rows); or NULL (y = LN(act(b))).
 * gamma / beta NULL: no LayerNorm (y = a + act(b)); else mean / rstd [M] are written for the
 * backward. 0 <= M < 2^31.
 * lgnn_res_norm_bwd: da, db (each nullable) [M][C] — db through the activation, da PER ROW also
 *   for a broadcast a (the caller sums the sets in fixed order: lgnn_reduce_partials with
 *   num_partials = M / a_rows, len = a_rows * C) — and, with gamma, the column sums
 *   part [2][num_partials][C] = (dgamma, dbeta) per workgroup in fixed order, each summed by
 *   lgnn_reduce_partials(.., num_partials, C); num_partials = lgnn_res_norm_bwd_partials(M).
 * ------------------------------------------------------------------------------------------- */
#define LGNN_ACT_RELU 2
int lgnn_res_norm_fwd(const float* a, int a_rows, const float* b, int act, const float* gamma,
                      const float* beta, float eps, int64_t M, int C, float* y, float* mean,
                      float* rstd, void* stream);
int lgnn_res_norm_bwd_partials(int64_t M);
int lgnn_res_norm_bwd(const float* a, int a_rows, const float* b, int act, const float* gamma,
                      int64_t M, int C, const float* mean, const float* rstd, const float* dy,
                      float* da, float* db, float* part, int num_partials, void* stream);

/* Set readout over x [num_sets * rows][C]. Replaces SetTransformerAggregation's
 * `x.nan_to_num()` + `x.flatten(1, 2) if concat else x.mean(dim=1)` (PyG set_transformer.py) and
 * the reference model's mean (set_transformer.py:64). mean = 1: out [num_sets][C] = the mean of a
 * set's rows; 0: out = x. gptr (nullable, int32 [num_sets + 1], the INPUT sets' offsets): a set
 * with no input row gives zeros (what nan_to_num leaves of PyG's fully masked softmax) and gets
 * zero gradient. lgnn_set_readout_bwd: dx [num_sets * rows][C]. */
int lgnn_set_readout_fwd(const float* x, const int32_t* gptr, int64_t num_sets, int rows, int C,
                         int mean, float* out, void* stream);
int lgnn_set_readout_bwd(const float* dout, const int32_t* gptr, int64_t num_sets, int rows,
                         int C, int mean, float* dx, void* stream);
/* y = a + b over n floats (y may alias a or b): where two gradient paths meet at a block's input
 * (the residual's and the projection's: autograd's AccumulateGrad add). */
int lgnn_add(const float* a, const float* b, float* y, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * PointNet++ (reference src/lesion_gnn/models/pointnet.py; PyG 2.5.1 PointNetConv, fps, radius,
 * global_max_pool; torch_cluster 1.6.3). The entries are additions: every earlier signature is
 * unchanged, so the ABI version stays.
 *
 * Geometry conventions as lgnn_knn_graph / lgnn_radius_graph: positions fp64 [rows][dims], dims 2
 * or 3 (fp32 positions widen exactly); squared distances fp64 with each operation rounded on its
 * own, so every selection is bit-exact against a float64 restatement; ptr int32 graph offsets;
 * nothing is allocated inside a call.
 *
 * lgnn_fps: farthest point sampling of every graph in one launch (torch_cluster.fps). ptr [B+1]
 *   the graphs' point offsets, optr [B+1] their output offsets (m_g = optr[g+1] - optr[g] picks,
 *   0 <= m_g <= n_g), start [B] the local index of each graph's first pick (in [0, n_g); ignored
 *   for an empty graph). idx [num_out = optr[B]] int64: global point indices in selection order.
 *   After each pick p, d[i] = min(d[i], |p_i - p_p|^2); the next pick is the argmax of d, lowest
 *   index on ties (all distinct positions taken: d is all zero and the graph's first point
 *   repeats, as torch_cluster does). One workgroup per graph; graphs of up to LGNN_FPS_CAPACITY
 *   points keep positions and distances in registers, larger ones use the workspace
 *   (lgnn_fps_workspace_bytes(N)).
 *
 * lgnn_radius_pairs_count / lgnn_radius_pairs: torch_cluster.radius(x, y, r, batch_x, batch_y,
 *   max_num_neighbors) — the bipartite form of lgnn_radius_graph: for every query y_i, walk the
 *   candidates x_j of its graph (ptr_x / ptr_y: the two sets' graph offsets) in index order and
 *   take j when |y_i - x_j|^2 < r * r, until max_num_neighbors are taken. pairs [2][E] int64 =
 *   (query i, candidate j), grouped by i, j ascending. _count leaves the int64 row offsets
 *   [Ny + 1] at the start of the workspace (lgnn_radius_pairs_workspace_bytes(Ny)); E is its last
 *   entry (the one host read).
 * lgnn_pairs_transpose: the candidate-grouped view of such a pair list: tptr [Nx + 1] int64 and
 *   perm [E] int64 with perm[tptr[j] .. tptr[j+1]) = the pairs whose candidate is j, ascending
 *   (count, scan, place by rank; no atomics). col = pairs + E, rowoff = the row offsets above.
 *   workspace: lgnn_pairs_transpose_workspace_bytes(Nx).
 * ------------------------------------------------------------------------------------------- */
#define LGNN_FPS_CAPACITY 1024
size_t lgnn_fps_workspace_bytes(int64_t num_nodes);
int lgnn_fps(const double* pos, int64_t num_nodes, int dims, const int32_t* ptr,
             const int32_t* optr, const int64_t* start, int64_t num_graphs, int64_t* idx,
             int64_t num_out, void* workspace, size_t workspace_bytes, void* stream);
size_t lgnn_radius_pairs_workspace_bytes(int64_t num_queries);
int lgnn_radius_pairs_count(const double* x, int64_t num_x, const double* y, int64_t num_y,
                            int dims, const int32_t* ptr_x, const int32_t* ptr_y,
                            int64_t num_graphs, double r, int max_num_neighbors, void* workspace,
                            size_t workspace_bytes, void* stream);
int lgnn_radius_pairs(const double* x, int64_t num_x, const double* y, int64_t num_y, int dims,
                      const int32_t* ptr_x, const int32_t* ptr_y, int64_t num_graphs, double r,
                      int max_num_neighbors, int64_t* pairs, int64_t num_pairs,
                      const void* workspace, size_t workspace_bytes, void* stream);
size_t lgnn_pairs_transpose_workspace_bytes(int64_t num_candidates);
int lgnn_pairs_transpose(const int64_t* col, const int64_t* rowoff, int64_t num_y,
                         int64_t num_pairs, const int32_t* ptr_x, const int32_t* ptr_y,
                         int64_t num_graphs, int64_t num_x, int64_t* tptr, int64_t* perm,
                         void* workspace, size_t workspace_bytes, void* stream);

/* PointNetConv's per-edge MLP input without a per-edge GEMM: with W1 = [Wx | Wp],
 *   cat[x_j, pos_j - pos_i] W1^T + b1 = U[j] - V[i],  U = cat[x, pos] W1^T + b1,  V = pos_i Wp^T.
 * lgnn_edge_sub_fwd: Z [E][C] = U[col[e]] - V[row[e]] and sums [2C] fp64 = (sum z, sum z^2) over
 *   the E rows, as lgnn_bn_stats leaves them (same partials, same fixed-order reduction), in one
 *   pass; workspace lgnn_bn_workspace_bytes(E, C). C % 4 == 0.
 * lgnn_segment_sum: out [S][C] = sign * sum_{k in [ptr[s], ptr[s+1])} X[perm ? perm[k] : k], fp32
 *   in ascending k — the backward of the above: dV = it(dZ, rowoff, NULL, -1), dU = it(dZ, tptr,
 *   perm, +1). Every output row is written; no atomics. C % 4 == 0.
 * lgnn_segment_max_fwd: out [S][C] = max over rows [ptr[s], ptr[s+1]) of X, arg [S][C] int32 the
 *   row that gave it (lowest on ties); an empty segment gives 0 and arg -1. PointNetConv's
 *   aggr='max' (segments = centroids, ptr = the pair row offsets) and global_max_pool (segments =
 *   graphs). Any C; fewer than 2^31 rows.
 * lgnn_segment_max_bwd: dX[e][c] = arg[seg(e)][c] == e ? dout[seg(e)][c] : 0 for every row of
 *   every segment (the segments tile X's rows: no memset, no scatter). */
int lgnn_edge_sub_fwd(const float* U, const float* V, const int64_t* row, const int64_t* col,
                      int64_t num_edges, int C, float* Z, double* sums, void* workspace,
                      size_t workspace_bytes, void* stream);
int lgnn_segment_sum(const float* X, const int64_t* ptr, const int64_t* perm,
                     int64_t num_segments, int C, float sign, float* out, void* stream);
int lgnn_segment_max_fwd(const float* X, const int64_t* ptr, int64_t num_segments, int C,
                         float* out, int32_t* arg, void* stream);
int lgnn_segment_max_bwd(const float* dout, const int32_t* arg, const int64_t* ptr,
                         int64_t num_segments, int C, float* dX, void* stream);

/* lgnn_bn_act / lgnn_bn_bwd_stats / lgnn_bn_bwd_apply with the activation as an argument:
 * LGNN_ACT_ELU (what those entries compute) or LGNN_ACT_RELU (PyG MLP's default act: the
 * PointNet++ MLPs). With scale = 1, shift = 0 and training = 0 they are act(Z) * mask and its
 * backward (an MLP layer without a norm). lgnn_bn_stats / lgnn_bn_finalize serve both. */
int lgnn_bn_act_a(const float* Z, int64_t M, int N, const float* scale, const float* shift,
                  const float* mask, int act, float* A, void* stream);
int lgnn_bn_bwd_stats_a(const float* dA, const float* Z, const float* mask, int64_t M, int N,
                        const float* scale, const float* shift, const float* mean,
                        const float* invstd, int act, double* sums, void* workspace,
                        size_t workspace_bytes, void* stream);
int lgnn_bn_bwd_apply_a(const float* dA, const float* Z, const float* mask, int64_t M, int N,
                        const float* scale, const float* shift, const float* mean,
                        const float* invstd, int act, const double* sums, double count,
                        int training, float* dZ, float* dgamma, float* dbeta, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Collation of a batch out of a device-resident graph dataset. Replaces: the per-step work of
 * torch_geometric.loader.DataLoader's Collater / Batch.from_data_list over the InMemoryDataset
 * (reference src/lesion_gnn/datasets/datamodule.py:63-69, datasets/base.py:27-115) for the
 * attributes x, pos, y, batch and ptr. The entries are additions: every earlier signature is
 * unchanged, so the ABI version stays.
 *   The dataset: x [rows, channels] fp32, pos [rows, dims] fp64 (dims 2 or 3; NULL: no positions,
 *   out_pos is not written), y [num_src_graphs] int64, src_ptr [num_src_graphs + 1] int64 (graph
 *   g owns rows [src_ptr[g], src_ptr[g + 1])). ids [num_sel] int64: the graphs of the batch, in
 *   batch order; repeats are legal.
 *   With n_b = src_ptr[ids[b] + 1] - src_ptr[ids[b]]: out_ptr [num_sel + 1] = the exclusive scan
 *   of n_b; out_batch[r] = b and out_x[out_ptr[b] + t] = x[src_ptr[ids[b]] + t] (out_pos
 *   likewise) for r = out_ptr[b] + t, t < n_b; out_y[b] = y[ids[b]].
 *   out_capacity: the rows out_x / out_pos / out_batch hold. The row total is read on the device
 *   (every device-side size is, so a captured call replays on refilled ids): rows at or beyond it
 *   are left untouched, and nothing is written at or beyond row out_capacity.
 *   err [1] int32, written: the number of ids outside [0, num_src_graphs) (each counts as an
 *   empty graph, out_y = -1), plus LGNN_COLLATE_OVERFLOW when the total exceeds out_capacity
 *   (out_ptr and out_y are complete all the same).
 *   out_x must be 16-byte aligned (all its stores are 16-byte stores); x, and the row width
 *   channels * 4, need not be. workspace: lgnn_collate_workspace_bytes(num_sel). num_sel = 0
 *   writes out_ptr[0] = 0 and err. Three launches (the gather is skipped when num_sel or
 *   out_capacity is 0), no host synchronisation. LGNN_EINVAL, before any launch: a negative count, channels < 1, dims not in
 *   {0, 2, 3}, a NULL required pointer, a workspace that is too small.
 * ------------------------------------------------------------------------------------------- */
#define LGNN_COLLATE_OVERFLOW 1073741824
size_t lgnn_collate_workspace_bytes(int64_t num_sel);
int lgnn_collate(const int64_t* ids, int64_t num_sel, const int64_t* src_ptr,
                 int64_t num_src_graphs, const float* x, int channels, const double* pos,
                 int dims, const int64_t* y, float* out_x, double* out_pos, int64_t* out_y,
                 int64_t* out_batch, int64_t* out_ptr, int64_t out_capacity, int32_t* err,
                 void* workspace, size_t workspace_bytes, void* stream);

/* lgnn_collate_edges: the edges of the same selection, for a dataset that keeps each graph's
 * edges (what PyG's Collater does to edge_index after the per-graph transforms, reference
 * datamodule.py:43-45,63-69). An addition: the ABI version stays.
 *   The dataset: edge_index [2, num_src_edges] int64 (row 0 the sources, row 1 the targets, ids
 *   the dataset's rows), src_edge_ptr [num_src_graphs + 1] int64 (graph g owns the edges
 *   [src_edge_ptr[g], src_edge_ptr[g + 1]), both endpoints in its rows), src_ptr as above;
 *   edge_weight [num_src_edges] of weight_bytes (4 or 8) bytes each, or NULL (weight_bytes is not
 *   read, out_edge_weight is not written). ids, num_sel as above; out_ptr [num_sel + 1]: the
 *   batch's row offsets as lgnn_collate wrote them for the same ids (same stream, or ordered
 *   after it).
 *   With g = ids[b] and m_b = src_edge_ptr[g + 1] - src_edge_ptr[g]: out_edge_ptr [num_sel + 1] =
 *   the exclusive scan of m_b; for t < m_b and j = out_edge_ptr[b] + t, out_edge_index[:, j] =
 *   edge_index[:, src_edge_ptr[g] + t] - src_ptr[g] + out_ptr[b] and out_edge_weight[j] = the
 *   source element, copied bit for bit.
 *   out_capacity: the edges out_edge_index [2, out_capacity] and out_edge_weight hold (the row
 *   stride of out_edge_index). The edge total is read on the device (a captured call replays on
 *   refilled ids): edges at or beyond it are left untouched, and nothing is written at or beyond
 *   edge out_capacity. A source position outside [0, num_src_edges) is skipped.
 *   err [1] int32, written: the number of ids outside [0, num_src_graphs) (each counts as a graph
 *   without edges), plus LGNN_COLLATE_OVERFLOW when the total exceeds out_capacity (out_edge_ptr
 *   is complete all the same).
 *   workspace: lgnn_collate_edges_workspace_bytes(num_sel), never 0. num_sel = 0 writes
 *   out_edge_ptr[0] = 0 and err. Three launches (the gather is skipped when num_sel,
 *   out_capacity or num_src_edges is 0), no host synchronisation. LGNN_EINVAL, before any
 *   launch: a negative count, a NULL required pointer, weights with weight_bytes not 4 or 8 or
 *   without out_edge_weight, a workspace that is too small. */
size_t lgnn_collate_edges_workspace_bytes(int64_t num_sel);
int lgnn_collate_edges(const int64_t* ids, int64_t num_sel, const int64_t* src_ptr,
                       const int64_t* src_edge_ptr, int64_t num_src_graphs,
                       const int64_t* edge_index, int64_t num_src_edges, const void* edge_weight,
                       int weight_bytes, const int64_t* out_ptr, int64_t* out_edge_index,
                       void* out_edge_weight, int64_t* out_edge_ptr, int64_t out_capacity,
                       int32_t* err, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * SIFT nodes for a batch of images of one size. Replaces: cv2.SIFT_create(nfeatures,
 * contrastThreshold = 0, sigma).detectAndCompute of the reference's SiftExtractor
 * (src/lesion_gnn/datasets/nodes/sift.py:50-52): OpenCV's algorithm with nOctaveLayers = 3 and
 * edgeThreshold = 10, restated (parity with OpenCV itself is not pinned). The
 * entries are additions: every earlier signature is unchanged, so the ABI version stays.
 *   Sizes: 1 <= batch <= 65535, height, width >= 2, batch * 24 * height * width < 2^31; sigma > 0
 *   with every blur radius <= LGNN_SIFT_MAX_RADIUS (sigma up to about 1.9). Anything else is
 *   LGNN_EINVAL before any launch, as are a NULL required pointer and a capacity or workspace
 *   that is too small.
 *   The pyramid: the image is doubled, so octave o is (2 * height >> o) x (2 * width >> o);
 *   lgnn_sift_num_octaves of them are built (those whose smaller side exceeds 10; 0 for sizes the
 *   entries refuse). The Gaussian buffer holds, octave after octave, [batch][6][h][w] fp32, the
 *   DoG buffer [batch][5][h][w]: lgnn_sift_pyramid_floats(batch, height, width) floats and 5/6 of
 *   that.
 * lgnn_sift_pyramid: image [batch, height, width, channels] uint8, channels 1 or 3 -> gray
 *   [batch, height, width] uint8 ((c0 * 1868 + c1 * 9617 + c2 * 4899 + 8192) >> 14: the
 *   reference's RGB array read as BGR) and both buffers. 1 + 6 launches per octave.
 * lgnn_sift_count: counts [rows] and row_ptr [rows + 1] int32, rows = lgnn_sift_rows(batch,
 *   height, width): one row per (image, octave, layer 1..3, row); row_ptr is the exclusive scan
 *   of the rows' 26-neighbour extrema at least 5 pixels from every edge, row_ptr[rows] their
 *   total (the caller reads it to size cand). Two launches.
 * lgnn_sift_candidates: cand [capacity, 5] int32 (image, octave, layer, row, column) in that
 *   order; nothing is written at or beyond row `capacity`. One launch.
 * lgnn_sift_keypoints: refinement (adjustLocalExtrema), orientation peaks, removal of keypoints
 *   equal in (pt, size, angle) to an earlier one, and the cut at the num_keypoints-th largest
 *   response (ties kept), per image; float64 on the fp32 levels. cand must be ordered by image;
 *   entries outside the pyramid are skipped. node_ptr [batch + 1] int64, written: the exclusive
 *   scan of the keypoints kept per image; the caller reads it to size the outputs. The rest
 *   stays in the workspace (lgnn_sift_keypoints_workspace_bytes(batch, num_candidates); 0 for
 *   counts the entry refuses) for lgnn_sift_gather. num_keypoints >= 1. Nine launches.
 * lgnn_sift_gather: the same workspace -> kf [total_nodes, 5] fp32 (x, y, size, angle, response;
 *   pt and size halved for the doubled image) and ki [total_nodes, 3] int32 (image, octave,
 *   layer), image by image, by response descending, then candidate order. One launch.
 * lgnn_sift_descriptors: kf, ki as above (any keypoints; entries outside the pyramid give a
 *   zero row) -> x [num_nodes, 128] fp32, integers in 0..255 (calcSIFTDescriptor), one wave per
 *   keypoint. One launch.
 * No float atomics: two calls give the same bits.
 * ------------------------------------------------------------------------------------------- */
#define LGNN_SIFT_MAX_OCTAVES 16
#define LGNN_SIFT_MAX_RADIUS 16
#define LGNN_SIFT_MAX_PEAKS 18
int lgnn_sift_num_octaves(int height, int width);
size_t lgnn_sift_pyramid_floats(int batch, int height, int width);
int lgnn_sift_pyramid(const uint8_t* image, int batch, int height, int width, int channels,
                      double sigma, uint8_t* gray, float* gauss, size_t gauss_floats, float* dog,
                      size_t dog_floats, void* stream);
size_t lgnn_sift_rows(int batch, int height, int width);
int lgnn_sift_count(const float* dog, int batch, int height, int width, int32_t* counts,
                    int32_t* row_ptr, void* stream);
int lgnn_sift_candidates(const float* dog, int batch, int height, int width,
                         const int32_t* row_ptr, int32_t* cand, int capacity, void* stream);
size_t lgnn_sift_keypoints_workspace_bytes(int batch, int num_candidates);
int lgnn_sift_keypoints(const float* gauss, const float* dog, int batch, int height, int width,
                        double sigma, const int32_t* cand, int num_candidates, int num_keypoints,
                        int64_t* node_ptr, void* workspace, size_t workspace_bytes, void* stream);
int lgnn_sift_gather(int batch, int num_candidates, const int64_t* node_ptr, int total_nodes,
                     float* kf, int32_t* ki, void* workspace, size_t workspace_bytes,
                     void* stream);
int lgnn_sift_descriptors(const float* gauss, int batch, int height, int width, const float* kf,
                          const int32_t* ki, int num_nodes, float* x, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fundus image preprocessing for a batch of uint8 RGB images of any sizes. Replaces the chain
 * FundusAutocrop -> LongestMaxSize -> PadIfNeeded(BORDER_CONSTANT) -> Normalize -> ToTensorV2 of
 * the reference (fundus_datamodules/base.py:93-120, utils/autocrop.py:28-45;
 * lesion_gnn/datasets/nodes/lesions.py:132-141), with OpenCV's 8-bit INTER_LINEAR and
 * INTER_NEAREST restated in integers (tests/fundus_ref.py states the arithmetic,
 * parity with OpenCV itself is not pinned). The entries are additions: every earlier signature
 * is unchanged, so the ABI version stays.
 *   images, masks: HOST arrays of `batch` device pointers, image b [heights[b], widths[b], 3] and
 *   mask b [heights[b], widths[b]] uint8, contiguous, at any byte alignment; heights, widths:
 *   host arrays. The tables are read during the call and packed into kernel arguments,
 *   LGNN_FUNDUS_MAX_IMAGES images per launch. No device allocation, no host read: capturable.
 *   LGNN_EINVAL, before any launch: batch < 1, a side outside [2, LGNN_FUNDUS_MAX_SIDE], size
 *   outside [2, LGNN_FUNDUS_MAX_SIDE], a std that is not > 0, a non-finite mean, a NULL table,
 *   image or required output, out and out_u8 both NULL, out_mask without masks (or a NULL mask
 *   among them).
 * lgnn_fundus_bbox: boxes [batch, 4] int32 (x_min, x_max, y_min, y_max): the extreme coordinates
 *   of the pixels with red > threshold (strict; a NaN threshold lights nothing), or (0, W, 0, H)
 *   when there is none or x_min == x_max or y_min == y_max. The crop image[y_min:y_max,
 *   x_min:x_max] excludes the last lit row and column, as the reference's does. One launch that
 *   zeroes the accumulators, then two per LGNN_FUNDUS_MAX_IMAGES images: a workgroup takes a
 *   contiguous share of lgnn_fundus_bbox_share(H, W) 16-pixel groups of its image (int32
 *   atomicMax across workgroups: order-free, so two calls give the same bits).
 * lgnn_fundus_bbox_share: that share for a height x width image, in 16-pixel groups counted from
 *   the image's first 16-byte-aligned byte: workgroup b reads groups [b * share, (b + 1) * share).
 *   0 for a side outside [2, LGNN_FUNDUS_MAX_SIDE]. A query: nothing is launched.
 * lgnn_fundus_preprocess: per image, from boxes[b] on the device: h = y_max - y_min, w = x_max -
 *   x_min; scale = size / double(max(h, w)); new_h = max(1, rint(h * scale)), new_w likewise
 *   (half to even, in double); the crop resized to new_h x new_w (INTER_LINEAR; the mask
 *   INTER_NEAREST); centred in size x size with pad_top = (size - new_h) / 2, pad_left likewise
 *   and the remainder below and right, padding 0; out[c][y][x] = (float(v) - m_c) * r_c with
 *   m_c = float(mean_c * 255), r_c = float(1 / (std_c * 255)) (products in double on the host).
 *   Nullable outputs: out [batch, 3, size, size] fp32, out_u8 [batch, size, size, 3] uint8
 *   (before the normalisation), out_mask [batch, size, size] uint8, geom [batch, 8] int32
 *   (x_min, y_min, w, h, new_w, new_h, pad_left, pad_top). boxes entries outside their image are
 *   clamped into it (no read outside an image whatever boxes holds). One launch per
 *   LGNN_FUNDUS_MAX_IMAGES images.
 * ------------------------------------------------------------------------------------------- */
#define LGNN_FUNDUS_MAX_SIDE 16384
#define LGNN_FUNDUS_MAX_IMAGES 16
int lgnn_fundus_bbox_share(int height, int width);
int lgnn_fundus_bbox(int batch, const uint8_t* const* images, const int* heights,
                     const int* widths, float threshold, int32_t* boxes, void* stream);
int lgnn_fundus_preprocess(int batch, const uint8_t* const* images, const uint8_t* const* masks,
                           const int* heights, const int* widths, const int32_t* boxes, int size,
                           double mean0, double mean1, double mean2, double std0, double std1,
                           double std2, float* out, uint8_t* out_u8, uint8_t* out_mask,
                           int32_t* geom, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LGNN_H */
