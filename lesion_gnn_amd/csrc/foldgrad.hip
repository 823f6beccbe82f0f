// The deferred in_proj fold of the fused GCN backward (stack3_bwd.hip, deferred mode): in_proj
// has no activation, so H_0 = X W_0^T + 1 b_0^T enters the first conv linearly and, with
// G_1 = Â^T dZ_1, T = G_1^T X ([w2][d_in]) and g = colsum G_1 ([w2]) summed over every closed
// tile of the step,
//   dW_0 = W_1^T T          [w1][d_in]
//   db_0 = W_1^T g          [w1]
//   dW_1 = T W_0^T + g b_0^T  [w2][w1]
// One launch per step from the reduced T and g: two products of at most 128^3 (4 MFLOP) as plain
// fp32 FMA chains (db_0's in double), every output element one thread's chain in index order (no
// atomics, the same bits on every run). The open tiles' directly formed totals are added when
// given.
#include "launch.h"

namespace {

constexpr int FT = 256;      // threads: 128 output columns x FR rows
constexpr int FR = 2;        // output rows per workgroup: one output element per thread
constexpr int FW = 128;      // widest layer
constexpr int FLD = FW + 4;  // padded row of the W_0 image (16-B reads of consecutive rows spread
                             // over the banks)
static_assert(FT == FW * FR, "one thread per output element");

struct FoldArgs {
  const float* T;   // [w2][d_in]
  const float* g;   // [w2]
  const float* W0;  // [w1][d_in]
  const float* b0;  // [w1]
  const float* W1;  // [w2][w1]
  const float* dW0_open;  // nullable: added
  const float* db0_open;
  const float* dW1_open;
  const int32_t* live;  // nullable: 0 = T and g are zero and unread (no closed tile)
  float* dW0;  // [w1][d_in]
  float* db0;  // [w1]
  float* dW1;  // [w2][w1]
  int d_in, w1, w2;
};

// rows * q 16-byte pieces (at most 4096 = 16 per thread) of dense global rows: the loads, all in
// flight at once (no address needs a division) ...
__device__ __forceinline__ void copy_load(f32x4 (&v)[16], const float* src, int n4) {
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int f = threadIdx.x + u * FT;
    v[u] = ld4(src + 4 * (int64_t)(f < n4 ? f : 0));  // (past the end: piece 0 again, not stored)
  }
}
// ... and their stores to LDS rows of ld floats: piece f = r q + p, stepped from thread to thread
// by FT = dr q + dp without a division per piece
__device__ __forceinline__ void copy_store(float* dst, int ld, const f32x4 (&v)[16], int n4,
                                           int q) {
  int r = threadIdx.x / q, p = threadIdx.x - r * q;
  const int dr = FT / q, dp = FT - dr * q;
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    if ((int)threadIdx.x + u * FT < n4) st4(dst + r * ld + 4 * p, v[u]);
    r += dr;
    p += dp;
    if (p >= q) {
      p -= q;
      ++r;
    }
  }
}

// workgroups [0, ceil(w1 / 2)): rows i0.. of dW_0 (and db_0); the rest: rows n0.. of dW_1; 128
// workgroups at the full widths. The launch is latency bound and every output element is one
// dependent chain, so the rows are spread thin: 2 per workgroup, one element per thread (8 rows
// as 4 chains per thread on 32 workgroups took 9.2 us). Everything a workgroup reads from
// global memory is issued up front, the 64 KiB operand first: one memory round trip. live
// (nullable): the closed-tile count of the backward launch; 0 = T and g are zero (and were not
// reduced): only the open totals.
__global__ __launch_bounds__(FT) void k_fold_wgrad(FoldArgs a) {
  __shared__ __attribute__((aligned(16))) float big[FW * FLD];  // T, or the padded W_0 image
  __shared__ __attribute__((aligned(16))) float strip[FR * FW];  // W_1 columns / T rows, [FR][FW]
  __shared__ float gs[FW];
  const int t = threadIdx.x;
  const int c = t & (FW - 1), rg = t >> 7;
  const int d_in = a.d_in, w1 = a.w1, w2 = a.w2;
  const int nb0 = (w1 + FR - 1) / FR;
  const int q = d_in / 4;  // 16-B pieces per row of T and W_0
  const bool role0 = (int)blockIdx.x < nb0;
  const int r0 = FR * (role0 ? (int)blockIdx.x : (int)blockIdx.x - nb0);  // first output row
  const int rows = role0 ? w1 : w2, cols = role0 ? d_in : w1;             // of the output
  const int r = r0 + rg;                                                  // this thread's row
  float* const out = role0 ? a.dW0 : a.dW1;
  const float* const open = role0 ? a.dW0_open : a.dW1_open;
  // (issued whether alive or not: the live word's own round trip is not waited for first)
  f32x4 v[16];
  copy_load(v, role0 ? a.T : a.W0, (role0 ? w2 : w1) * q);
  const bool alive = !a.live || a.live[0] != 0;  // uniform
  // dead, and the open totals are the outputs themselves (as the training step passes them):
  // they are the result already. The workgroup ends with its operand loads still in flight
  if (!alive && open == out && (!role0 || a.db0_open == a.db0)) return;
  // this thread's open total (row r, column c), db_0's, g, b_0
  const float ov = (open && c < cols && r < rows) ? open[(int64_t)r * cols + c] : 0.f;
  const bool dbt = role0 && t < FR && r0 + t < w1;  // this thread forms db_0[r0 + t]
  const float obv = (a.db0_open && dbt) ? a.db0_open[r0 + t] : 0.f;
  float acc = 0.f;
  double dbs = 0.0;
  if (alive) {
    const float gv = t < w2 ? a.g[t] : 0.f;
    if (role0) {
      // W_1's columns r0, r0 + 1 as [2][n] (thread t: row t / 2, column t % 2: 8 bytes of a
      // row from a lane pair); T whole ([w2][d_in], dense)
      const int sn = t >> 1, si = r0 + (t & 1);
      const float sv = (sn < w2 && si < w1) ? a.W1[(int64_t)sn * w1 + si] : 0.f;
      copy_store(big, d_in, v, w2 * q, q);
      strip[FW * (t & 1) + sn] = sv;
      if (t < FW) gs[t] = gv;
      __syncthreads();
      const int kc = c < d_in ? c : 0;
#pragma unroll 2
      for (int n = 0; n < w2; n += 4) {  // w2 % 4 == 0
        const f32x4 wv = ld4(strip + FW * rg + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fmaf(wv[e], big[(n + e) * d_in + kc], acc);
      }
      if (dbt) {
        // db_0 sums w2 products of mixed sign whose total is far below their magnitudes (g is a
        // column sum over every node): the chains run in double (128 x 128 FMAs per step), so
        // the only rounding left is g's own and the final one. Four interleaved chains, n mod 4,
        // combined in a fixed order: the latency of one
        double s4[4] = {0.0, 0.0, 0.0, 0.0};
        for (int n = 0; n < w2; n += 4) {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            s4[e] = fma((double)strip[FW * t + n + e], (double)gs[n + e], s4[e]);
        }
        dbs = (s4[0] + s4[1]) + (s4[2] + s4[3]);
      }
    } else {
      // T's rows r0, r0 + 1 as [2][128] (FR q <= 64 pieces), b_0; W_0 ([w1][d_in]) as padded rows
      const int sr = t / q, sp = t - sr * q;
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      const f32x4 sv =
          (sr < FR && r0 + sr < w2) ? ld4(a.T + (int64_t)(r0 + sr) * d_in + 4 * sp) : z;
      const float bv = c < w1 ? a.b0[c] : 0.f;
      copy_store(big, FLD, v, w1 * q, q);
      if (sr < FR) st4(strip + FW * sr + 4 * sp, sv);
      if (t < FW) gs[t] = gv;
      __syncthreads();
      const int ic = c < w1 ? c : 0;
#pragma unroll 4
      for (int p = 0; p < q; ++p) {
        const f32x4 wv = ld4(big + ic * FLD + 4 * p);
        const f32x4 tv = ld4(strip + FW * rg + 4 * p);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fmaf(tv[e], wv[e], acc);
      }
      acc = fmaf(gs[r & (FW - 1)], bv, acc);
    }
  }
  if (c < cols && r < rows) out[(int64_t)r * cols + c] = open ? acc + ov : acc;
  if (dbt) a.db0[r0 + t] = (float)(a.db0_open ? dbs + (double)obv : dbs);
}

}  // namespace

extern "C" int lgnn_gcn_fold_wgrad(const float* T, const float* g, const float* W0,
                                   const float* b0, const float* W1, int d_in, int w1, int w2,
                                   const float* dW0_open, const float* db0_open,
                                   const float* dW1_open, const int32_t* live, float* dW0,
                                   float* db0, float* dW1, void* stream) {
  if (!T || !g || !W0 || !b0 || !W1 || !dW0 || !db0 || !dW1) return LGNN_EINVAL;
  for (const int w : {d_in, w1, w2})
    if (w < 4 || w > FW || w % 4 != 0) return LGNN_EINVAL;
  FoldArgs a = {T, g, W0, b0, W1, dW0_open, db0_open, dW1_open, live, dW0, db0, dW1, d_in, w1, w2};
  const unsigned grid = (unsigned)((w1 + FR - 1) / FR + (w2 + FR - 1) / FR);
  return launch(k_fold_wgrad, dim3(grid), dim3(FT), as_stream(stream), a);
}
