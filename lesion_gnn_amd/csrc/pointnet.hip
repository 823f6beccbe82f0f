// PointNetConv pieces (PyG 2.5.1 PointNetConv(local_nn, aggr='max'), reference
// src/lesion_gnn/models/pointnet.py SAModule / GlobalSAModule) around the dense GEMMs:
//
//   lgnn_edge_sub_fwd   Z[e] = U[col[e]] - V[row[e]] — the first Linear of the per-edge MLP,
//                       cat[x_j, pos_j - pos_i] W1^T + b1, split into node-level products
//                       U = cat[x, pos] W1^T + b1 and V = pos[idx] Wp^T, so no [E, c_in + dims]
//                       operand exists — with the BatchNorm column sums (sum z, sum z^2; fp64
//                       partials per 256 rows, reduced in fixed order by lgnn_bn_partials_reduce)
//                       formed in the same pass.
//   lgnn_segment_sum    out[s] = sign * sum_{k in [ptr[s], ptr[s+1])} X[perm ? perm[k] : k]: the
//                       backward of the above (dV = -row sums of dZ; dU = sums over the
//                       candidate-grouped permutation of lgnn_pairs_transpose, ascending pair
//                       order). No atomics.
//   lgnn_segment_max_*  PointNetConv's max aggregation and global_max_pool, with the argmax saved
//                       for a backward that writes every element of dX.
//
// Thread mapping of the 4-column kernels as norm.hip: 32 lanes x 4 consecutive columns cover a
// 128-column chunk (blockIdx.y), the block's 8 half-wave row groups stride rows / segments.
#include "launch.h"

namespace {

constexpr int NT = 256;
constexpr int RG = NT / 32;
constexpr int ROWS_PER_BLOCK = 256;  // as lgnn_bn_stats: lgnn_bn_workspace_bytes sizes the partials

inline int row_blocks(int64_t M) {
  const int64_t b = (M + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  return (int)(b < 1 ? 1 : b);
}

__global__ __launch_bounds__(NT) void k_edge_sub(const float* __restrict__ U,
                                                 const float* __restrict__ V,
                                                 const int64_t* __restrict__ row,
                                                 const int64_t* __restrict__ col, int64_t E,
                                                 int C, float* __restrict__ Z,
                                                 double* __restrict__ part) {
  __shared__ double red[2][RG][128];
  const int li = threadIdx.x & 31, rg = threadIdx.x >> 5;
  const int c = blockIdx.y * 128 + 4 * li;
  const int64_t e0 = (int64_t)blockIdx.x * ROWS_PER_BLOCK;
  const int64_t e1 = e0 + ROWS_PER_BLOCK < E ? e0 + ROWS_PER_BLOCK : E;
  double s0[4] = {0.0, 0.0, 0.0, 0.0}, s1[4] = {0.0, 0.0, 0.0, 0.0};
  if (c < C) {
    for (int64_t e = e0 + rg; e < e1; e += RG) {
      const f32x4 z = ld4(U + col[e] * C + c) - ld4(V + row[e] * C + c);
      st4(Z + e * C + c, z);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s0[j] += (double)z[j];
        s1[j] += (double)z[j] * (double)z[j];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    red[0][rg][4 * li + j] = s0[j];
    red[1][rg][4 * li + j] = s1[j];
  }
  __syncthreads();
  const int k = threadIdx.x >> 7, cl = threadIdx.x & 127;  // (sum kind, column), groups in order
  const int cc = blockIdx.y * 128 + cl;
  double t = red[k][0][cl];
#pragma unroll
  for (int g = 1; g < RG; ++g) t += red[k][g][cl];
  if (cc < C) part[(int64_t)blockIdx.x * 2 * C + k * C + cc] = t;
}

__global__ __launch_bounds__(NT) void k_segment_sum(const float* __restrict__ X,
                                                    const int64_t* __restrict__ ptr,
                                                    const int64_t* __restrict__ perm, int64_t S,
                                                    int C, float sign, float* __restrict__ out) {
  const int li = threadIdx.x & 31, rg = threadIdx.x >> 5;
  const int c = blockIdx.y * 128 + 4 * li;
  if (c >= C) return;
  for (int64_t s = (int64_t)blockIdx.x * RG + rg; s < S; s += (int64_t)gridDim.x * RG) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int64_t k = ptr[s]; k < ptr[s + 1]; ++k) acc += ld4(X + (perm ? perm[k] : k) * C + c);
    st4(out + s * C + c, acc * sign);
  }
}

// one thread per (segment, column): 4 segments x 64 columns per block, any C
constexpr int MC = 64;
constexpr int MS = NT / MC;

__global__ __launch_bounds__(NT) void k_segment_max_fwd(const float* __restrict__ X,
                                                        const int64_t* __restrict__ ptr,
                                                        int64_t S, int C, float* __restrict__ out,
                                                        int32_t* __restrict__ arg) {
  const int c = blockIdx.y * MC + (threadIdx.x & (MC - 1));
  if (c >= C) return;
  for (int64_t s = (int64_t)blockIdx.x * MS + threadIdx.x / MC; s < S;
       s += (int64_t)gridDim.x * MS) {
    const int64_t e0 = ptr[s], e1 = ptr[s + 1];
    float best = 0.f;
    int64_t at = -1;
    for (int64_t e = e0; e < e1; ++e) {  // ascending: a strict > keeps the lowest row on ties
      const float v = X[e * C + c];
      if (at < 0 || v > best) {
        best = v;
        at = e;
      }
    }
    out[s * C + c] = best;
    arg[s * C + c] = (int32_t)at;
  }
}

__global__ __launch_bounds__(NT) void k_segment_max_bwd(const float* __restrict__ dout,
                                                        const int32_t* __restrict__ arg,
                                                        const int64_t* __restrict__ ptr,
                                                        int64_t S, int C,
                                                        float* __restrict__ dX) {
  const int c = blockIdx.y * MC + (threadIdx.x & (MC - 1));
  if (c >= C) return;
  for (int64_t s = (int64_t)blockIdx.x * MS + threadIdx.x / MC; s < S;
       s += (int64_t)gridDim.x * MS) {
    const int64_t at = arg[s * C + c];
    const float g = dout[s * C + c];
    for (int64_t e = ptr[s]; e < ptr[s + 1]; ++e) dX[e * C + c] = e == at ? g : 0.f;
  }
}

inline dim3 seg_grid(int64_t S, int per_block, int C, int chunk) {
  int64_t g = (S + per_block - 1) / per_block;
  if (g > 4096) g = 4096;
  return dim3((unsigned)(g < 1 ? 1 : g), (unsigned)((C + chunk - 1) / chunk));
}

}  // namespace

extern "C" int lgnn_edge_sub_fwd(const float* U, const float* V, const int64_t* row,
                                 const int64_t* col, int64_t E, int C, float* Z, double* sums,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  if (E < 0 || C <= 0 || (C & 3) || !sums || E > INT32_MAX) return LGNN_EINVAL;
  if (E > 0 && (!U || !V || !row || !col || !Z)) return LGNN_EINVAL;
  if (!workspace || workspace_bytes < lgnn_bn_workspace_bytes(E, C)) return LGNN_ENOSPC;
  const int P = row_blocks(E);
  double* part = static_cast<double*>(workspace);
  if (const int e = launch(k_edge_sub, dim3(P, (C + 127) / 128), dim3(NT), as_stream(stream), U, V,
                           row, col, E, C, Z, part)) return e;
  return lgnn_bn_partials_reduce(part, P, C, sums, nullptr, nullptr, stream);
}

extern "C" int lgnn_segment_sum(const float* X, const int64_t* ptr, const int64_t* perm,
                                int64_t S, int C, float sign, float* out, void* stream) {
  if (S < 0 || C <= 0 || (C & 3)) return LGNN_EINVAL;
  if (S == 0) return LGNN_OK;
  if (!X || !ptr || !out) return LGNN_EINVAL;
  return launch(k_segment_sum, seg_grid(S, RG, C, 128), dim3(NT), as_stream(stream), X, ptr, perm,
                S, C, sign, out);
}

extern "C" int lgnn_segment_max_fwd(const float* X, const int64_t* ptr, int64_t S, int C,
                                    float* out, int32_t* arg, void* stream) {
  if (S < 0 || C <= 0) return LGNN_EINVAL;
  if (S == 0) return LGNN_OK;
  if (!ptr || !out || !arg) return LGNN_EINVAL;
  return launch(k_segment_max_fwd, seg_grid(S, MS, C, MC), dim3(NT), as_stream(stream), X, ptr, S,
                C, out, arg);
}

extern "C" int lgnn_segment_max_bwd(const float* dout, const int32_t* arg, const int64_t* ptr,
                                    int64_t S, int C, float* dX, void* stream) {
  if (S < 0 || C <= 0) return LGNN_EINVAL;
  if (S == 0) return LGNN_OK;
  if (!dout || !arg || !ptr) return LGNN_EINVAL;
  return launch(k_segment_max_bwd, seg_grid(S, MS, C, MC), dim3(NT), as_stream(stream), dout, arg,
                ptr, S, C, dX);
}
