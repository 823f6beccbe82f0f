// Radius graph construction on the GPU for a batch of graphs: torch_cluster.radius_graph(pos, r,
// batch, loop, max_num_neighbors, flow='source_to_target') as PyG 2.5.1's RadiusGraph transform
// calls it — the connectivity the reference's sweep offers beside KNNGraph
// (src/lesion_gnn/scripts/sweep.py:113-118: RadiusGraph(r), r in [1, 1536] pixels; transforms.py:19-23
// resolves it by name). torch_cluster is not under /root/reference; its published algorithm
// (1.6.3, radius_cuda.cu + radius.py) is restated here:
//   radius_graph: limit = loop ? max_num_neighbors : max_num_neighbors + 1; radius(x, x, r, ...)
//   radius:       for every query q of graph g, walk the candidates c of g in INDEX order and take
//                 c when |p_q - p_c|^2 < r * r (strict), stopping once `limit` are taken
//   radius_graph: edge_index = [c, q] (source_to_target), and without `loop` the self pair is
//                 removed afterwards — so a query whose first `limit` in-range candidates do not
//                 include itself keeps max_num_neighbors + 1 neighbours, as torch_cluster does.
// The neighbour choice when more than `limit` candidates are in range is torch_cluster's CUDA
// one (the first `limit` in index order); its CPU path (nanoflann, unsorted radius search) keeps
// a traversal-dependent subset — documented, parity unpinned there (oracle/pyg_ref.py).
// Squared distances: fp64 dx*dx + dy*dy (+ dz*dz) with each operation rounded on its own, the
// arithmetic of the oracle's restatement ((p_q - p_c)**2).sum(-1), so edge lists are bit-exact.
//
// Two passes with one host read between them (the edge count sizes the output):
//   lgnn_radius_count:  per-query neighbour counts, then their exclusive scan (int64 offsets in
//                       the workspace; offsets[N] = the edge count);
//   lgnn_radius_graph:  the same walk again, each query writing its edges at offsets[q].
// Layout: pos [N][D] fp64 (D = 2 or 3), ptr [B+1] int32 graph offsets (Batch.ptr), batch [N]
// int64 sorted. One thread per query; a block's queries are consecutive nodes, so the candidates
// of its graphs are one contiguous node range, staged through LDS in chunks (as k_knn).
#include "launch.h"
#include "geom.h"
#include "wg.h"

namespace {

constexpr int QT = 256;      // queries (threads) per block
constexpr int CHUNK = 1024;  // candidates staged per round

// WRITE = false: cnt[q] = the query's edge count; WRITE = true: its edges at off[q]
template <int D, bool WRITE>
__global__ __launch_bounds__(QT) void k_radius(const double* __restrict__ pos, int64_t N,
                                               const int64_t* __restrict__ batch,
                                               const int32_t* __restrict__ ptr, double r2,
                                               int limit, int loop, int32_t* __restrict__ cnt,
                                               const int64_t* __restrict__ off, int64_t E,
                                               int64_t* __restrict__ ei) {
  __shared__ double cp[CHUNK * D];
  const int64_t q0 = (int64_t)blockIdx.x * QT;
  const int64_t q = q0 + threadIdx.x;
  const int64_t qlast = q0 + QT - 1 < N - 1 ? q0 + QT - 1 : N - 1;
  const int64_t cbeg = ptr[batch[q0]], cend = ptr[batch[qlast] + 1];
  const bool active = q < N;
  int64_t gs = 0, ge = 0;
  double pq[D];
  if (active) {
    const int64_t g = batch[q];
    gs = ptr[g];
    ge = ptr[g + 1];
#pragma unroll
    for (int d = 0; d < D; ++d) pq[d] = pos[q * D + d];
  }
  int taken = 0;    // candidates taken by the walk (self included), <= limit
  int64_t w = 0;    // edges written (WRITE)
  const int64_t base = WRITE && active ? off[q] : 0;
  for (int64_t c0 = cbeg; c0 < cend; c0 += CHUNK) {
    const int64_t c1 = c0 + CHUNK < cend ? c0 + CHUNK : cend;
    // every query of the block has taken `limit` candidates, or its graph ends before this
    // chunk: the rest of the range cannot add an edge (block-uniform, so the barriers stay so)
    if (!__syncthreads_or(active && taken < limit && ge > c0)) break;
    for (int64_t i = c0 * D + threadIdx.x; i < c1 * D; i += QT) cp[i - c0 * D] = pos[i];
    __syncthreads();
    if (!active || taken >= limit) continue;
    const int64_t lo = gs > c0 ? gs : c0, hi = ge < c1 ? ge : c1;
    for (int64_t c = lo; c < hi && taken < limit; ++c) {
      if (sqd(pq, cp + (c - c0) * D, D) < r2) {
        ++taken;
        if (!loop && c == q) continue;  // removed by radius_graph after the walk
        if constexpr (WRITE) {
          if (base + w < E) {  // E = offsets[N] (lgnn_radius_count); a short buffer is not overrun
            ei[base + w] = c;
            ei[E + base + w] = q;
          }
        }
        ++w;
      }
    }
  }
  if constexpr (!WRITE) {
    if (active) cnt[q] = (int32_t)w;
  }
}

struct RadiusWs {
  int64_t* off;  // [N + 1]
  int32_t* cnt;  // [N]
};

RadiusWs radius_ws(void* ws, int64_t N) {
  RadiusWs r;
  r.off = static_cast<int64_t*>(ws);
  r.cnt = reinterpret_cast<int32_t*>(r.off + N + 1);
  return r;
}

int radius_args_ok(const double* pos, int64_t N, int dims, const int64_t* batch,
                   const int32_t* ptr, int64_t B, double r, int max_num_neighbors) {
  if (N < 0 || B < 0 || (dims != 2 && dims != 3) || !(r >= 0.0) || max_num_neighbors < 1)
    return 0;
  if (N > 0 && (!pos || !batch || !ptr)) return 0;
  if (N > 0 && B == 0) return 0;  // nodes but no graphs: batch cannot index ptr
  if (N > INT32_MAX) return 0;
  return 1;
}

}  // namespace

extern "C" size_t lgnn_radius_workspace_bytes(int64_t num_nodes) {
  if (num_nodes < 0) return 0;
  return (size_t)(num_nodes + 1) * sizeof(int64_t) + (size_t)num_nodes * sizeof(int32_t);
}

extern "C" int lgnn_radius_count(const double* pos, int64_t N, int dims, const int64_t* batch,
                                 const int32_t* ptr, int64_t B, double r, int max_num_neighbors,
                                 int loop, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  if (!radius_args_ok(pos, N, dims, batch, ptr, B, r, max_num_neighbors)) return LGNN_EINVAL;
  if (!workspace || workspace_bytes < lgnn_radius_workspace_bytes(N)) return LGNN_ENOSPC;
  hipStream_t s = as_stream(stream);
  const RadiusWs w = radius_ws(workspace, N);
  if (N == 0) {
    if (hipMemsetAsync(w.off, 0, sizeof(int64_t), s) != hipSuccess) return (int)hipGetLastError();
    return LGNN_OK;
  }
  const double r2 = r * r;  // torch_cluster squares r on the host, in double
  const int limit = loop ? max_num_neighbors : max_num_neighbors + 1;
  const dim3 grid((unsigned)((N + QT - 1) / QT));
  one_of<3, 2>(dims, [&](auto D) {
    enqueue(k_radius<D, false>, grid, dim3(QT), s, pos, N, batch, ptr, r2, limit, loop, w.cnt,
            nullptr, 0, nullptr);
  });
  if (const int e = last_error()) return e;
  launch_exclusive_scan(w.cnt, N, w.off, s);
  return last_error();
}

extern "C" int lgnn_radius_graph(const double* pos, int64_t N, int dims, const int64_t* batch,
                                 const int32_t* ptr, int64_t B, double r, int max_num_neighbors,
                                 int loop, int64_t* edge_index, int64_t num_edges,
                                 const void* workspace, size_t workspace_bytes, void* stream) {
  if (!radius_args_ok(pos, N, dims, batch, ptr, B, r, max_num_neighbors)) return LGNN_EINVAL;
  if (num_edges < 0 || (num_edges > 0 && !edge_index)) return LGNN_EINVAL;
  if (!workspace || workspace_bytes < lgnn_radius_workspace_bytes(N)) return LGNN_ENOSPC;
  if (N == 0 || num_edges == 0) return LGNN_OK;
  hipStream_t s = as_stream(stream);
  const RadiusWs w = radius_ws(const_cast<void*>(workspace), N);
  const double r2 = r * r;
  const int limit = loop ? max_num_neighbors : max_num_neighbors + 1;
  const dim3 grid((unsigned)((N + QT - 1) / QT));
  one_of<3, 2>(dims, [&](auto D) {
    enqueue(k_radius<D, true>, grid, dim3(QT), s, pos, N, batch, ptr, r2, limit, loop, nullptr,
            w.off, num_edges, edge_index);
  });
  return last_error();
}

// ------------------------------------------------------------------------------------------
// Bipartite form: torch_cluster.radius(x, y, r, batch_x, batch_y, max_num_neighbors) — the queries
// y (PointNet++: the FPS centroids, in selection order) and the candidates x are different point
// sets over the same graphs. Same walk, same arithmetic, same two passes as above; no self pair
// to drop. The queries of a block are consecutive query rows, hence of consecutive graphs, so
// their candidates are the contiguous range ptr_x[first graph] .. ptr_x[last graph + 1], staged
// through LDS in chunks. A query's graph is found in ptr_y (queries carry no batch vector).
// ------------------------------------------------------------------------------------------
namespace {

// the graph g with ptr[g] <= i < ptr[g + 1] (the last g with ptr[g] <= i: empty graphs skipped)
__device__ __forceinline__ int graph_of(const int32_t* __restrict__ ptr, int B, int64_t i) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (ptr[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

template <int D, bool WRITE>
__global__ __launch_bounds__(QT) void k_radius_pairs(const double* __restrict__ x,
                                                     const double* __restrict__ y, int64_t Ny,
                                                     const int32_t* __restrict__ ptrx,
                                                     const int32_t* __restrict__ ptry, int B,
                                                     double r2, int limit,
                                                     int32_t* __restrict__ cnt,
                                                     const int64_t* __restrict__ off, int64_t E,
                                                     int64_t* __restrict__ pairs) {
  __shared__ double cp[CHUNK * D];
  const int64_t q0 = (int64_t)blockIdx.x * QT;
  const int64_t q = q0 + threadIdx.x;
  const int64_t qlast = q0 + QT - 1 < Ny - 1 ? q0 + QT - 1 : Ny - 1;
  const int64_t cbeg = ptrx[graph_of(ptry, B, q0)], cend = ptrx[graph_of(ptry, B, qlast) + 1];
  const bool active = q < Ny;
  int64_t gs = 0, ge = 0;
  double pq[D];
  if (active) {
    const int g = graph_of(ptry, B, q);
    gs = ptrx[g];
    ge = ptrx[g + 1];
#pragma unroll
    for (int d = 0; d < D; ++d) pq[d] = y[q * D + d];
  }
  int taken = 0;
  const int64_t base = WRITE && active ? off[q] : 0;
  for (int64_t c0 = cbeg; c0 < cend; c0 += CHUNK) {
    const int64_t c1 = c0 + CHUNK < cend ? c0 + CHUNK : cend;
    if (!__syncthreads_or(active && taken < limit && ge > c0)) break;
    for (int64_t i = c0 * D + threadIdx.x; i < c1 * D; i += QT) cp[i - c0 * D] = x[i];
    __syncthreads();
    if (!active || taken >= limit) continue;
    const int64_t lo = gs > c0 ? gs : c0, hi = ge < c1 ? ge : c1;
    for (int64_t c = lo; c < hi && taken < limit; ++c) {
      if (sqd(pq, cp + (c - c0) * D, D) < r2) {
        if constexpr (WRITE) {
          if (base + taken < E) {  // E = offsets[Ny]: a short buffer is not overrun
            pairs[base + taken] = q;
            pairs[E + base + taken] = c;
          }
        }
        ++taken;
      }
    }
  }
  if constexpr (!WRITE) {
    if (active) cnt[q] = taken;
  }
}

int pairs_args_ok(const double* x, int64_t Nx, const double* y, int64_t Ny, int dims,
                  const int32_t* ptrx, const int32_t* ptry, int64_t B, double r,
                  int max_num_neighbors) {
  if (Nx < 0 || Ny < 0 || B < 0 || (dims != 2 && dims != 3) || !(r >= 0.0) ||
      max_num_neighbors < 1)
    return 0;
  if (Nx > INT32_MAX || Ny > INT32_MAX || B > INT32_MAX) return 0;
  if ((Nx > 0 && !x) || (Ny > 0 && !y)) return 0;
  if (Ny > 0 && (B == 0 || !ptrx || !ptry)) return 0;
  return 1;
}

// Transpose of a pair list grouped by query with ascending candidates: per candidate j the pairs
// naming it, in ascending pair order. One thread per candidate: it walks the query rows of its
// graph and looks j up in each row's ascending candidate list (binary search; a row holds at most
// max_num_neighbors). PLACE = false: cnt[j]; true: perm[tptr[j] + rank] = pair index. No atomics.
template <bool PLACE>
__global__ __launch_bounds__(QT) void k_pairs_transpose(const int64_t* __restrict__ col,
                                                        const int64_t* __restrict__ rowoff,
                                                        const int32_t* __restrict__ ptrx,
                                                        const int32_t* __restrict__ ptry, int B,
                                                        int64_t Nx, int32_t* __restrict__ cnt,
                                                        const int64_t* __restrict__ tptr,
                                                        int64_t* __restrict__ perm) {
  const int64_t j = (int64_t)blockIdx.x * QT + threadIdx.x;
  if (j >= Nx) return;
  const int g = graph_of(ptrx, B, j);
  int64_t w = PLACE ? tptr[j] : 0;
  int n = 0;
  for (int64_t i = ptry[g]; i < ptry[g + 1]; ++i) {
    int64_t lo = rowoff[i], hi = rowoff[i + 1];
    while (lo < hi) {  // the first pair of row i with col >= j
      const int64_t mid = (lo + hi) >> 1;
      if (col[mid] < j) lo = mid + 1; else hi = mid;
    }
    if (lo < rowoff[i + 1] && col[lo] == j) {
      if constexpr (PLACE) perm[w++] = lo;
      ++n;
    }
  }
  if constexpr (!PLACE) cnt[j] = n;
}

}  // namespace

extern "C" size_t lgnn_radius_pairs_workspace_bytes(int64_t num_queries) {
  return lgnn_radius_workspace_bytes(num_queries);
}

extern "C" int lgnn_radius_pairs_count(const double* x, int64_t Nx, const double* y, int64_t Ny,
                                       int dims, const int32_t* ptr_x, const int32_t* ptr_y,
                                       int64_t B, double r, int max_num_neighbors,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  if (!pairs_args_ok(x, Nx, y, Ny, dims, ptr_x, ptr_y, B, r, max_num_neighbors))
    return LGNN_EINVAL;
  if (!workspace || workspace_bytes < lgnn_radius_workspace_bytes(Ny)) return LGNN_ENOSPC;
  hipStream_t s = as_stream(stream);
  const RadiusWs w = radius_ws(workspace, Ny);
  if (Ny == 0) {
    if (hipMemsetAsync(w.off, 0, sizeof(int64_t), s) != hipSuccess) return (int)hipGetLastError();
    return LGNN_OK;
  }
  const double r2 = r * r;
  const dim3 grid((unsigned)((Ny + QT - 1) / QT));
  one_of<3, 2>(dims, [&](auto D) {
    enqueue(k_radius_pairs<D, false>, grid, dim3(QT), s, x, y, Ny, ptr_x, ptr_y, (int)B, r2,
            max_num_neighbors, w.cnt, nullptr, 0, nullptr);
  });
  if (const int e = last_error()) return e;
  launch_exclusive_scan(w.cnt, Ny, w.off, s);
  return last_error();
}

extern "C" int lgnn_radius_pairs(const double* x, int64_t Nx, const double* y, int64_t Ny,
                                 int dims, const int32_t* ptr_x, const int32_t* ptr_y, int64_t B,
                                 double r, int max_num_neighbors, int64_t* pairs,
                                 int64_t num_pairs, const void* workspace,
                                 size_t workspace_bytes, void* stream) {
  if (!pairs_args_ok(x, Nx, y, Ny, dims, ptr_x, ptr_y, B, r, max_num_neighbors))
    return LGNN_EINVAL;
  if (num_pairs < 0 || (num_pairs > 0 && !pairs)) return LGNN_EINVAL;
  if (!workspace || workspace_bytes < lgnn_radius_workspace_bytes(Ny)) return LGNN_ENOSPC;
  if (Ny == 0 || num_pairs == 0) return LGNN_OK;
  const RadiusWs w = radius_ws(const_cast<void*>(workspace), Ny);
  const double r2 = r * r;
  const dim3 grid((unsigned)((Ny + QT - 1) / QT));
  hipStream_t s = as_stream(stream);
  one_of<3, 2>(dims, [&](auto D) {
    enqueue(k_radius_pairs<D, true>, grid, dim3(QT), s, x, y, Ny, ptr_x, ptr_y, (int)B, r2,
            max_num_neighbors, nullptr, w.off, num_pairs, pairs);
  });
  return last_error();
}

extern "C" size_t lgnn_pairs_transpose_workspace_bytes(int64_t num_candidates) {
  return num_candidates > 0 ? (size_t)num_candidates * sizeof(int32_t) : 0;
}

extern "C" int lgnn_pairs_transpose(const int64_t* col, const int64_t* rowoff, int64_t Ny,
                                    int64_t num_pairs, const int32_t* ptr_x,
                                    const int32_t* ptr_y, int64_t B, int64_t Nx, int64_t* tptr,
                                    int64_t* perm, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  if (Nx < 0 || Ny < 0 || B < 0 || num_pairs < 0 || !tptr || Nx > INT32_MAX || B > INT32_MAX)
    return LGNN_EINVAL;
  if (Nx > 0 && (B == 0 || !ptr_x || !ptr_y || !rowoff)) return LGNN_EINVAL;
  if (num_pairs > 0 && (!col || !perm || Nx == 0)) return LGNN_EINVAL;
  if (Nx > 0 && (!workspace || workspace_bytes < lgnn_pairs_transpose_workspace_bytes(Nx)))
    return LGNN_ENOSPC;
  hipStream_t s = as_stream(stream);
  if (Nx == 0) {
    if (hipMemsetAsync(tptr, 0, sizeof(int64_t), s) != hipSuccess) return (int)hipGetLastError();
    return LGNN_OK;
  }
  int32_t* cnt = static_cast<int32_t*>(workspace);
  const dim3 grid((unsigned)((Nx + QT - 1) / QT));
  if (const int e = launch(k_pairs_transpose<false>, grid, dim3(QT), s, col, rowoff, ptr_x, ptr_y,
                           (int)B, Nx, cnt, nullptr, nullptr)) return e;
  launch_exclusive_scan(cnt, Nx, tptr, s);
  if (const int e = last_error()) return e;
  if (num_pairs > 0) {
    if (const int e = launch(k_pairs_transpose<true>, grid, dim3(QT), s, col, rowoff, ptr_x, ptr_y,
                             (int)B, Nx, nullptr, tptr, perm)) return e;
  }
  return LGNN_OK;
}
