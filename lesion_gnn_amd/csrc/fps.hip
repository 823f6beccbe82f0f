// Farthest point sampling of every graph of a batch in one launch: torch_cluster.fps(pos, batch,
// ratio, random_start) as PyG's PointNet++ set-abstraction module calls it (reference
// src/lesion_gnn/models/pointnet.py SAModule). torch_cluster 1.6.3's rule (fps_cuda.cu), restated:
//   the first pick of graph g is ptr[g] + start[g]; after each pick p every point keeps
//   d[i] = min(d[i], |p_i - p_p|^2); the next pick is the argmax of d, the lowest index on ties.
// Once every distinct position is taken d is all zero and the graph's first point repeats.
// Squared distances as radius.hip: fp64, each operation rounded on its own, so the picks are
// bit-exact against the float64 restatement ((p - p_pick) ** 2).sum(-1).
//
// One workgroup per graph. Graphs of up to LGNN_FPS_CAPACITY points keep their positions and
// running minimum distances in registers (PER points per thread, point i on thread i % FT);
// larger graphs keep d in the caller's workspace and re-read pos. Per pick: a wave reduction of
// (d, index) and one cross-wave step through LDS (double-buffered: one barrier per pick).
#include "launch.h"
#include "geom.h"

namespace {

constexpr int FT = 256;                        // threads per graph
constexpr int PER = LGNN_FPS_CAPACITY / FT;    // on-chip points per thread
constexpr int WAVES = FT / 64;
static_assert(LGNN_FPS_CAPACITY % FT == 0, "capacity is a whole number of points per thread");

struct Best {
  double d;
  int i;
};

// a farther point wins; at equal distance the lower index
__device__ __forceinline__ bool beats(double d, int i, const Best& b) {
  return d > b.d || (d == b.d && i < b.i);
}

// p: the graph's points [n][D]; out: its m picks (global indices base + local); dws: its n
// workspace distances (!ONCHIP)
template <int D, bool ONCHIP>
__device__ void fps_graph(const double* __restrict__ p, int n, int m, int pick, int64_t base,
                          int64_t* __restrict__ out, double* __restrict__ dws,
                          Best (*red)[WAVES]) {
  const int t = threadIdx.x;
  double d[PER], q[PER][D];
  if constexpr (ONCHIP) {
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = t + k * FT;
      d[k] = __builtin_inf();
#pragma unroll
      for (int a = 0; a < D; ++a) q[k][a] = i < n ? p[(int64_t)i * D + a] : 0.0;
    }
  } else {
    for (int i = t; i < n; i += FT) dws[i] = __builtin_inf();
  }
  for (int j = 0; j < m; ++j) {
    if (t == 0) out[j] = base + pick;
    if (j + 1 == m) break;
    double c[D];
#pragma unroll
    for (int a = 0; a < D; ++a) c[a] = p[(int64_t)pick * D + a];
    Best b = {-1.0, INT32_MAX};
    if constexpr (ONCHIP) {
#pragma unroll
      for (int k = 0; k < PER; ++k) {  // ascending i: a strict > keeps the lowest index
        const int i = t + k * FT;
        if (i < n) {
          d[k] = fmin(d[k], sqd(q[k], c, D));
          if (d[k] > b.d) b = {d[k], i};
        }
      }
    } else {
      for (int i = t; i < n; i += FT) {
        const double v = fmin(dws[i], sqd(p + (int64_t)i * D, c, D));
        dws[i] = v;
        if (v > b.d) b = {v, i};
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double od = __shfl_xor(b.d, off);
      const int oi = __shfl_xor(b.i, off);
      if (beats(od, oi, b)) b = {od, oi};
    }
    Best* r = red[j & 1];
    if ((t & 63) == 0) r[t >> 6] = b;
    __syncthreads();
    b = r[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w)
      if (beats(r[w].d, r[w].i, b)) b = r[w];
    pick = b.i;
  }
}

template <int D>
__global__ __launch_bounds__(FT) void k_fps(const double* __restrict__ pos,
                                            const int32_t* __restrict__ ptr,
                                            const int32_t* __restrict__ optr,
                                            const int64_t* __restrict__ start,
                                            int64_t* __restrict__ idx, double* __restrict__ dws) {
  __shared__ Best red[2][WAVES];
  const int g = blockIdx.x;
  const int64_t n0 = ptr[g], o0 = optr[g];
  const int n = ptr[g + 1] - ptr[g], m = optr[g + 1] - optr[g];
  if (n <= 0 || m <= 0) return;  // block-uniform
  int64_t s = start[g];
  s = s < 0 ? 0 : s >= n ? n - 1 : s;  // a start outside the graph cannot index outside it
  if (n <= LGNN_FPS_CAPACITY)
    fps_graph<D, true>(pos + n0 * D, n, m, (int)s, n0, idx + o0, nullptr, red);
  else
    fps_graph<D, false>(pos + n0 * D, n, m, (int)s, n0, idx + o0, dws + n0, red);
}

}  // namespace

extern "C" size_t lgnn_fps_workspace_bytes(int64_t num_nodes) {
  return num_nodes > 0 ? (size_t)num_nodes * sizeof(double) : 0;
}

extern "C" int lgnn_fps(const double* pos, int64_t N, int dims, const int32_t* ptr,
                        const int32_t* optr, const int64_t* start, int64_t B, int64_t* idx,
                        int64_t num_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (N < 0 || B < 0 || num_out < 0 || (dims != 2 && dims != 3) || N > INT32_MAX ||
      B > INT32_MAX)
    return LGNN_EINVAL;
  if (B > 0 && (!ptr || !optr || !start)) return LGNN_EINVAL;
  if (N > 0 && !pos) return LGNN_EINVAL;
  if (num_out > 0 && (!idx || N == 0 || B == 0)) return LGNN_EINVAL;
  if (N > 0 && (!workspace || workspace_bytes < lgnn_fps_workspace_bytes(N))) return LGNN_ENOSPC;
  if (B == 0 || num_out == 0) return LGNN_OK;
  hipStream_t s = as_stream(stream);
  double* dws = static_cast<double*>(workspace);
  one_of<3, 2>(dims, [&](auto D) {
    enqueue(k_fps<D>, dim3((unsigned)B), dim3(FT), s, pos, ptr, optr, start, idx, dws);
  });
  return last_error();
}
