// Collation of a selection of graphs out of a device-resident dataset (lgnn_collate): PyG's
// Collater / Batch.from_data_list for x, pos, y, batch and ptr (reference
// src/lesion_gnn/datasets/datamodule.py:63-69, a DataLoader over the InMemoryDataset of
// datasets/base.py:27-115), as three launches with no host read.
//
// k_collate_sizes (one thread per selected graph): n_b = src_ptr[ids[b] + 1] - src_ptr[ids[b]],
// the graph's first source row and out_y. k_collate_scan (one workgroup): out_ptr = the
// exclusive scan of n_b, the row shift delta[b] = src_ptr[ids[b]] - out_ptr[b] (workspace), err.
//
// k_collate_gather: a graph's rows are contiguous in the source and in the output, so inside
// graph b the output float f is the source float f + delta[b] * channels. The work is cut by
// bytes, not by graph: workgroup c owns the output floats [c * kChunk, (c + 1) * kChunk) of
// out_x, whatever graphs they fall in (a graph is 4 KB to 2 MB at 1025 channels). It finds the
// graphs of its first and last row by a 256-way search of out_ptr (two or three rounds, one
// probe per thread); each thread then bisects that short range for its first row and keeps the
// graph, its end and its shift in registers for the rows that follow.
// Every store of out_x is a 16-byte store at a 16-byte aligned address. The row width need not be
// a multiple of 16 bytes (4100 at 1025 channels), so the source of such a store sits at any
// 4-byte offset m: the thread loads the two aligned 16-byte vectors that hold its four floats
// and picks them out in registers (m = 0: the one vector twice). Both vectors hold at least one
// float of the graph, so no load leaves the 16-byte lines the graph's own floats are in. Four
// such pairs are in flight per thread before the first is stored. A vector that spans two
// graphs, or the end of the rows, is done float by float. The grid is sized from out_capacity;
// the row count is read on the device (out_ptr[num_sel]), and workgroups past it return at once.
// The last workgroups of the grid do the per-row outputs (out_batch, out_pos), kRows rows each.
#include "launch.h"
#include "wg.h"

namespace {

constexpr int kT = 256;
constexpr int kVecs = 8;                   // 16-byte stores per thread
constexpr int kGroup = 4;                  // of which this many are in flight at once
constexpr int kChunk = kT * kVecs * 4;     // floats of out_x per workgroup (32 KB)
constexpr int kRowsPer = 4;                // rows per thread in a row workgroup
constexpr int kRows = kT * kRowsPer;
constexpr int kScanT = 1024;

// Per selected graph b: its size into out_ptr[b] (-1 for an id outside the dataset, or a
// negative size), its first source row into delta[b], its label. One thread per graph over as
// many workgroups as that takes: three uncoalesced reads per graph, too many for one CU's
// memory pipeline at 10000 graphs.
__global__ __launch_bounds__(kT) void k_collate_sizes(
    const int64_t* __restrict__ ids, int64_t num_sel, const int64_t* __restrict__ src_ptr,
    int64_t num_src, const int64_t* __restrict__ y, int64_t* __restrict__ out_y,
    int64_t* __restrict__ out_ptr, int64_t* __restrict__ delta) {
  const int64_t b = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (b >= num_sel) return;
  const int64_t id = ids[b];
  const bool ok = id >= 0 && id < num_src;
  const int64_t first = ok ? src_ptr[id] : 0;
  const int64_t n = ok ? src_ptr[id + 1] - first : -1;
  out_ptr[b] = n >= 0 ? n : -1;
  delta[b] = first;
  out_y[b] = ok ? y[id] : -1;
}

// One workgroup: out_ptr from the sizes to their exclusive scan, delta from the first source
// row to the row shift, in tiles of kScanT graphs (thread t owns graph tile + t: coalesced, and
// no thread reads what another wrote), the total and err.
__global__ __launch_bounds__(kScanT) void k_collate_scan(
    int64_t num_sel, int64_t* __restrict__ out_ptr, int64_t* __restrict__ delta,
    int64_t capacity, int32_t* __restrict__ err) {
  __shared__ int64_t s_wave[kScanT / 64];
  const int t = threadIdx.x;
  int64_t carry = 0, bad = 0;
  int64_t next = t < num_sel ? out_ptr[t] : 0;
  for (int64_t tile = 0; tile < num_sel; tile += kScanT) {
    const int64_t b = tile + t;
    const int64_t raw = next;
    next = b + kScanT < num_sel ? out_ptr[b + kScanT] : 0;  // in flight during this tile's scan
    bad += __syncthreads_count(raw < 0);
    const int64_t at = block_exclusive_scan<kScanT>(raw > 0 ? raw : (int64_t)0, carry, s_wave);
    if (b < num_sel) {
      out_ptr[b] = at;
      delta[b] -= at;
    }
  }
  if (t == 0) {
    out_ptr[num_sel] = carry;
    const int64_t nb = bad < LGNN_COLLATE_OVERFLOW ? bad : LGNN_COLLATE_OVERFLOW - 1;
    err[0] = (int32_t)((unsigned)nb | (carry > capacity ? (unsigned)LGNN_COLLATE_OVERFLOW : 0u));
  }
}

// The last b in [0, num_sel) with out_ptr[b] <= r, for 0 <= r < out_ptr[num_sel]: the graph of
// output row r (empty graphs before it are passed over). Uniform: every thread of the workgroup
// calls it with the same r. Each round probes kT evenly spaced entries of the open range.
__device__ __forceinline__ int64_t graph_of_row_wg(const int64_t* __restrict__ out_ptr,
                                                   int64_t num_sel, int64_t r) {
  int64_t lo = 0, hi = num_sel;
  while (hi - lo > 1) {
    const int64_t step = (hi - lo + kT - 1) / kT;
    const int64_t i = lo + (int64_t)threadIdx.x * step;
    const int hit = i < hi && out_ptr[i] <= r;
    const int c = __syncthreads_count(hit);  // >= 1: out_ptr[lo] <= r
    lo += (int64_t)(c - 1) * step;
    hi = lo + step < hi ? lo + step : hi;
  }
  return lo;
}

// the same by bisection of [lo, hi], one thread's own row
__device__ __forceinline__ int64_t graph_of_row(const int64_t* __restrict__ out_ptr, int64_t lo,
                                                int64_t hi, int64_t r) {
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (out_ptr[mid] <= r) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Four floats from p, which is 4-byte aligned: the two aligned vectors around them (the one
// vector twice when p is aligned, so that neither load leaves the floats' own 16-byte lines),
// and the four picked out of the pair.
struct Pair {
  f32x4 a, b;
};
__device__ __forceinline__ Pair ld_pair(const float* p) {
  const unsigned m = ((unsigned)(uintptr_t)p >> 2) & 3u;
  const float* pa = p - m;
  return {ld4(pa), ld4(pa + (m ? 4 : 0))};
}
__device__ __forceinline__ f32x4 realign(const Pair& v, const float* p) {
  const unsigned m = ((unsigned)(uintptr_t)p >> 2) & 3u;
  const f32x4 a = v.a, b = v.b;
  f32x4 r;
  r.x = m == 0u ? a.x : m == 1u ? a.y : m == 2u ? a.z : a.w;
  r.y = m == 0u ? a.y : m == 1u ? a.z : m == 2u ? a.w : b.x;
  r.z = m == 0u ? a.z : m == 1u ? a.w : m == 2u ? b.x : b.y;
  r.w = m == 0u ? a.w : m == 1u ? b.x : m == 2u ? b.y : b.z;
  return r;
}

__global__ __launch_bounds__(kT) void k_collate_gather(
    const float* __restrict__ x, int channels, const double* __restrict__ pos, int dims,
    const int64_t* __restrict__ out_ptr, const int64_t* __restrict__ delta, int64_t num_sel,
    float* __restrict__ out_x, double* __restrict__ out_pos, int64_t* __restrict__ out_batch,
    int64_t capacity, int64_t x_blocks) {
  const int64_t total = out_ptr[num_sel];
  const int64_t rows = total < capacity ? total : capacity;  // nothing at or beyond either
  const int64_t blk = blockIdx.x;
  const unsigned ch = (unsigned)channels;
  if (blk >= x_blocks) {
    // per-row outputs
    const int64_t r0 = (blk - x_blocks) * kRows;
    if (r0 >= rows) return;
    const int64_t r1 = r0 + kRows < rows ? r0 + kRows : rows;
    const int64_t g_lo = graph_of_row_wg(out_ptr, num_sel, r0);
    const int64_t g_hi = graph_of_row_wg(out_ptr, num_sel, r1 - 1);
#pragma unroll
    for (int u = 0; u < kRowsPer; ++u) {
      const int64_t r = r0 + u * kT + threadIdx.x;
      if (r >= r1) break;
      const int64_t g = graph_of_row(out_ptr, g_lo, g_hi, r);
      out_batch[r] = g;
      if (pos) {
        const int64_t sr = r + delta[g];
        for (int d = 0; d < dims; ++d) out_pos[r * dims + d] = pos[sr * dims + d];
      }
    }
    return;
  }
  const int64_t f0 = blk * kChunk;  // this workgroup's first float of out_x
  const int64_t lim = rows * ch;    // floats of out_x to write
  if (f0 >= lim) return;
  const int64_t f1 = f0 + kChunk < lim ? f0 + kChunk : lim;
  const int64_t r0 = f0 / ch;
  const unsigned c0 = (unsigned)(f0 - r0 * ch);
  const int64_t g_lo = graph_of_row_wg(out_ptr, num_sel, r0);
  const int64_t g_hi = graph_of_row_wg(out_ptr, num_sel, (f1 - 1) / ch);
  // A thread's vectors are 4 KB apart and in row order, so most of them fall in the graph of the
  // one before: that graph, its end row and its shift stay in registers (gc, end_c, shift_c) and
  // out_ptr is searched again only past the end.
  int64_t gc = g_lo, end_c = -1, shift_c = 0;
  // kGroup vectors at a time: their graphs found, then all their loads issued, then the stores
#pragma unroll
  for (int u0 = 0; u0 < kVecs; u0 += kGroup) {
    int64_t src[kGroup];  // the 16-byte path's first source float; -1: none, or float by float
    int64_t gs[kGroup];
#pragma unroll
    for (int i = 0; i < kGroup; ++i) {
      const unsigned o = (unsigned)((u0 + i) * kT + threadIdx.x) * 4u;  // offset in the chunk
      const int64_t f = f0 + o;
      src[i] = -1;
      gs[i] = -1;
      if (f >= f1) continue;
      // rows of the first and the last float, relative to r0 (32-bit: o + c0 < kChunk + channels)
      const unsigned q = (o + c0) / ch, rem = (o + c0) - q * ch;
      const unsigned q3 = rem + 3u < ch ? q : q + (rem + 3u) / ch;
      if (r0 + q >= end_c) {
        gc = graph_of_row(out_ptr, gc, g_hi, r0 + q);
        end_c = out_ptr[gc + 1];
        shift_c = delta[gc] * (int64_t)ch;
      }
      gs[i] = gc;
      // one graph holds all four floats: its end is past the last float's row
      if (f + 3 < f1 && end_c > r0 + q3) src[i] = f + shift_c;
    }
    Pair v[kGroup];
#pragma unroll
    for (int i = 0; i < kGroup; ++i)
      if (src[i] >= 0) v[i] = ld_pair(x + src[i]);
#pragma unroll
    for (int i = 0; i < kGroup; ++i) {
      const unsigned o = (unsigned)((u0 + i) * kT + threadIdx.x) * 4u;
      const int64_t f = f0 + o;
      if (src[i] >= 0) {
        st4(out_x + f, realign(v[i], x + src[i]));
        continue;
      }
      if (gs[i] < 0) continue;
      float w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        w[j] = 0.f;
        if (f + j < f1) {
          const int64_t gj = graph_of_row(out_ptr, gs[i], g_hi, r0 + (o + c0 + j) / ch);
          w[j] = x[f + j + delta[gj] * (int64_t)ch];
        }
      }
      if (f + 3 < f1) {
        f32x4 w4 = {w[0], w[1], w[2], w[3]};
        st4(out_x + f, w4);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (f + j < f1) out_x[f + j] = w[j];
      }
    }
  }
}

// ---- edges (lgnn_collate_edges) ---------------------------------------------------------------
// A store that keeps each graph's edges (GraphStore.with_edges) has them contiguous per graph, so
// inside selected graph b the output edge j is the source edge j + edelta[b], and both endpoints
// move by shift[b] = out_ptr[b] - src_ptr[ids[b]]. Three launches, shaped as the three above:
// k_collate_edge_sizes (one thread per selected graph), k_collate_scan itself for out_edge_ptr,
// and k_collate_edge_gather, cut by output edges, not by graph: workgroup c owns the output edges
// [c * kEdgeChunk, (c + 1) * kEdgeChunk) whatever graphs they fall in (a graph has 0 to a few
// thousand edges; a workgroup per graph would idle 255 lanes on a one-edge graph and serialise a
// 3000-edge one). It finds the graphs of its first and last edge with graph_of_row_wg, each thread
// bisects that short range. Thread t's u-th edge is c * kEdgeChunk + u * kT + t, so every wave
// store of either row is 64 consecutive int64 (512 B); the loads are as contiguous as the graphs
// are. An edge's source position is at any 8-byte offset, so 16-byte accesses would need the
// pairing of k_collate_gather for a payload 100 times smaller than x: not done.

constexpr int kEdgesPer = 4;               // edges per thread, all loads in flight before a store
constexpr int kEdgeChunk = kT * kEdgesPer;

// Per selected graph b: its edge count into out_edge_ptr[b] (-1 for an id outside the dataset or
// a negative count), its first source edge into efirst[b], its endpoint shift into shift[b].
__global__ __launch_bounds__(kT) void k_collate_edge_sizes(
    const int64_t* __restrict__ ids, int64_t num_sel, const int64_t* __restrict__ src_ptr,
    const int64_t* __restrict__ src_edge_ptr, int64_t num_src, const int64_t* __restrict__ out_ptr,
    int64_t* __restrict__ out_edge_ptr, int64_t* __restrict__ efirst,
    int64_t* __restrict__ shift) {
  const int64_t b = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (b >= num_sel) return;
  const int64_t id = ids[b];
  const bool ok = id >= 0 && id < num_src;
  const int64_t first = ok ? src_edge_ptr[id] : 0;
  const int64_t m = ok ? src_edge_ptr[id + 1] - first : -1;
  out_edge_ptr[b] = m >= 0 ? m : -1;
  efirst[b] = first;
  shift[b] = ok ? out_ptr[b] - src_ptr[id] : 0;
}

template <typename W>
__global__ __launch_bounds__(kT) void k_collate_edge_gather(
    const int64_t* __restrict__ edge_index, int64_t num_src_edges, const W* __restrict__ weight,
    const int64_t* __restrict__ out_edge_ptr, const int64_t* __restrict__ edelta,
    const int64_t* __restrict__ shift, int64_t num_sel, int64_t* __restrict__ out_edge_index,
    W* __restrict__ out_weight, int64_t capacity) {
  const int64_t total = out_edge_ptr[num_sel];
  const int64_t edges = total < capacity ? total : capacity;  // nothing at or beyond either
  const int64_t j0 = (int64_t)blockIdx.x * kEdgeChunk;
  if (j0 >= edges) return;
  const int64_t j1 = j0 + kEdgeChunk < edges ? j0 + kEdgeChunk : edges;
  const int64_t g_lo = graph_of_row_wg(out_edge_ptr, num_sel, j0);
  const int64_t g_hi = graph_of_row_wg(out_edge_ptr, num_sel, j1 - 1);
  int64_t src[kEdgesPer], sh[kEdgesPer];
  int64_t gc = g_lo;
#pragma unroll
  for (int u = 0; u < kEdgesPer; ++u) {
    const int64_t j = j0 + u * kT + threadIdx.x;
    src[u] = -1;
    sh[u] = 0;
    if (j >= j1) continue;
    gc = graph_of_row(out_edge_ptr, gc, g_hi, j);  // a thread's edges ascend
    const int64_t e = j + edelta[gc];
    if (e >= 0 && e < num_src_edges) src[u] = e;  // a src_edge_ptr beyond edge_index reads nothing
    sh[u] = shift[gc];
  }
  int64_t s[kEdgesPer], t[kEdgesPer];
  W w[kEdgesPer];
#pragma unroll
  for (int u = 0; u < kEdgesPer; ++u) {
    if (src[u] < 0) continue;
    s[u] = edge_index[src[u]];
    t[u] = edge_index[num_src_edges + src[u]];
    if (weight) w[u] = weight[src[u]];
  }
#pragma unroll
  for (int u = 0; u < kEdgesPer; ++u) {
    if (src[u] < 0) continue;
    const int64_t j = j0 + u * kT + threadIdx.x;
    out_edge_index[j] = s[u] + sh[u];
    out_edge_index[capacity + j] = t[u] + sh[u];
    if (weight) out_weight[j] = w[u];
  }
}

}  // namespace

extern "C" size_t lgnn_collate_workspace_bytes(int64_t num_sel) {
  return num_sel > 0 ? (size_t)num_sel * sizeof(int64_t) : 0;
}

extern "C" int lgnn_collate(const int64_t* ids, int64_t num_sel, const int64_t* src_ptr,
                            int64_t num_src_graphs, const float* x, int channels,
                            const double* pos, int dims, const int64_t* y, float* out_x,
                            double* out_pos, int64_t* out_y, int64_t* out_batch, int64_t* out_ptr,
                            int64_t out_capacity, int32_t* err, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (num_sel < 0 || num_src_graphs < 0 || out_capacity < 0 || channels < 1 ||
      channels > (1 << 30) || (dims != 0 && dims != 2 && dims != 3))
    return LGNN_EINVAL;
  if (!out_ptr || !err || !src_ptr) return LGNN_EINVAL;
  if (num_sel > 0 && (!ids || !y || !out_y || !workspace)) return LGNN_EINVAL;
  if (num_sel > 0 && out_capacity > 0 && (!x || !out_x || !out_batch)) return LGNN_EINVAL;
  if (pos && (dims == 0 || !out_pos)) return LGNN_EINVAL;
  if (((uintptr_t)out_x & 15u) != 0) return LGNN_EINVAL;
  if (workspace_bytes < lgnn_collate_workspace_bytes(num_sel)) return LGNN_EINVAL;
  // the gather's grid covers out_capacity rows
  const int64_t max_floats = INT64_MAX / 2;
  if (out_capacity > max_floats / channels) return LGNN_EINVAL;
  const int64_t x_blocks = (out_capacity * channels + kChunk - 1) / kChunk;
  const int64_t row_blocks = (out_capacity + kRows - 1) / kRows;
  if (x_blocks + row_blocks > 0x7fffffff) return LGNN_EINVAL;
  int64_t* delta = static_cast<int64_t*>(workspace);
  if (num_sel > 0) {
    if ((num_sel + kT - 1) / kT > 0x7fffffff) return LGNN_EINVAL;
    if (const int e = launch(k_collate_sizes, dim3((unsigned)((num_sel + kT - 1) / kT)), dim3(kT),
                             as_stream(stream), ids, num_sel, src_ptr, num_src_graphs, y, out_y,
                             out_ptr, delta)) return e;
  }
  if (const int e = launch(k_collate_scan, dim3(1), dim3(kScanT), as_stream(stream), num_sel,
                           out_ptr, delta, out_capacity, err)) return e;
  if (num_sel == 0 || out_capacity == 0) return LGNN_OK;
  return launch(k_collate_gather, dim3((unsigned)(x_blocks + row_blocks)), dim3(kT),
                as_stream(stream), x, channels, pos, dims, out_ptr, delta, num_sel, out_x, out_pos,
                out_batch, out_capacity, x_blocks);
}

extern "C" size_t lgnn_collate_edges_workspace_bytes(int64_t num_sel) {
  // efirst / edelta [num_sel] and shift [num_sel]; never 0, so that a caller's buffer has an address
  return ((size_t)(num_sel > 0 ? num_sel : 0) * 2 + 2) * sizeof(int64_t);
}

extern "C" int lgnn_collate_edges(const int64_t* ids, int64_t num_sel, const int64_t* src_ptr,
                                  const int64_t* src_edge_ptr, int64_t num_src_graphs,
                                  const int64_t* edge_index, int64_t num_src_edges,
                                  const void* edge_weight, int weight_bytes,
                                  const int64_t* out_ptr, int64_t* out_edge_index,
                                  void* out_edge_weight, int64_t* out_edge_ptr,
                                  int64_t out_capacity, int32_t* err, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  if (num_sel < 0 || num_src_graphs < 0 || num_src_edges < 0 || out_capacity < 0)
    return LGNN_EINVAL;
  if (!out_edge_ptr || !err || !src_ptr || !src_edge_ptr || !workspace) return LGNN_EINVAL;
  if (num_sel > 0 && (!ids || !out_ptr)) return LGNN_EINVAL;
  if (num_sel > 0 && out_capacity > 0 && num_src_edges > 0 && (!edge_index || !out_edge_index))
    return LGNN_EINVAL;
  if (edge_weight && ((weight_bytes != 4 && weight_bytes != 8) || !out_edge_weight))
    return LGNN_EINVAL;
  if (workspace_bytes < lgnn_collate_edges_workspace_bytes(num_sel)) return LGNN_EINVAL;
  const int64_t blocks = (out_capacity + kEdgeChunk - 1) / kEdgeChunk;
  if (blocks > 0x7fffffff || (num_sel + kT - 1) / kT > 0x7fffffff) return LGNN_EINVAL;
  int64_t* edelta = static_cast<int64_t*>(workspace);
  int64_t* shift = edelta + num_sel;
  if (num_sel > 0) {
    if (const int e = launch(k_collate_edge_sizes, dim3((unsigned)((num_sel + kT - 1) / kT)),
                             dim3(kT), as_stream(stream), ids, num_sel, src_ptr, src_edge_ptr,
                             num_src_graphs, out_ptr, out_edge_ptr, edelta, shift)) return e;
  }
  if (const int e = launch(k_collate_scan, dim3(1), dim3(kScanT), as_stream(stream), num_sel,
                           out_edge_ptr, edelta, out_capacity, err)) return e;
  if (num_sel == 0 || out_capacity == 0 || num_src_edges == 0) return LGNN_OK;
  if (edge_weight && weight_bytes == 8)
    hipLaunchKernelGGL(k_collate_edge_gather<uint64_t>, dim3((unsigned)blocks), dim3(kT), 0,
                       as_stream(stream), edge_index, num_src_edges,
                       static_cast<const uint64_t*>(edge_weight), out_edge_ptr, edelta, shift,
                       num_sel, out_edge_index, static_cast<uint64_t*>(out_edge_weight),
                       out_capacity);
  else
    hipLaunchKernelGGL(k_collate_edge_gather<uint32_t>, dim3((unsigned)blocks), dim3(kT), 0,
                       as_stream(stream), edge_index, num_src_edges,
                       static_cast<const uint32_t*>(edge_weight), out_edge_ptr, edelta, shift,
                       num_sel, out_edge_index, static_cast<uint32_t*>(out_edge_weight),
                       out_capacity);
  return last_error();
}
