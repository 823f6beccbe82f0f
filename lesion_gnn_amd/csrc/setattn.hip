// Set attention for gfx950: segmented multi-head attention over ragged sets, the residual +
// activation + LayerNorm of a multihead attention block, and the set readout.
// Replaces the hot path of PyG 2.5.1 torch_geometric/nn/aggr/utils.py (MultiheadAttentionBlock,
// SetAttentionBlock, InducedSetAttentionBlock, PoolingByMultiheadAttention) and set_transformer.py
// (SetTransformerAggregation), which the reference model src/lesion_gnn/models/set_transformer.py
// :16-66 builds on: there every set is padded to the longest (to_dense_batch) and masked; here a
// set's rows are the contiguous range its pointer delimits, so there is no padded row, no mask and
// no [B, Nmax, Nmax] score tensor.
//
// Attention: kSplit workgroups per (set, head), each owning every kSplit-th block (a long set is
// shared out, a short one leaves the others idle at once). Forward: for each block of
// LGNN_SET_ATTN_QROWS query rows, the key/value rows stream through LDS in blocks of
// LGNN_SET_ATTN_KROWS with a running max and sum per query row (online softmax); only the output
// and one log-sum-exp per (query row, head) reach memory. Backward: P recomputed from q, k and the
// saved log-sum-exp, in two launches: dK / dV per key block (in registers over all query blocks)
// and dQ per query block (in registers over all key blocks). Every output element has one owner
// and one fixed summation order: no atomics, two runs agree bit for bit.
// The products run on the fp32 VALU (fmaf chains): on gfx950 the fp32 MFMA has the VALU's rate,
// and bf16 operands would not hold the 1e-4 bar without a split.
#include "launch.h"
#include "wg.h"

namespace lgnn_setattn {

constexpr int kThreads = 256;
constexpr int QB = LGNN_SET_ATTN_QROWS;
constexpr int KB = LGNN_SET_ATTN_KROWS;
constexpr int PLD = KB + 1;  // row stride of the probability tiles
constexpr int kSplit = 8;    // workgroups per (set, head): each owns every kSplit-th block
static_assert(QB == 16 && KB == 32, "the thread maps below are written for 16 x 32 tiles");

struct Args {
  const float* q;
  const float* k;
  const float* v;
  int64_t ldq, ldk, ldv;
  const int32_t* qptr;
  const int32_t* kptr;
  int q_rows, q_shared, k_rows;
  int H, D;
  float scale;
  const float* mask;
  const int64_t* moff;
};

// rows [start, start + n) of set g: ragged by ptr, or `rows` per set
__device__ __forceinline__ void segment(const int32_t* ptr, int rows, int64_t g, int64_t& start,
                                        int& n) {
  if (ptr) {
    start = ptr[g];
    n = ptr[g + 1] - ptr[g];
  } else {
    start = g * rows;
    n = rows;
  }
  if (n < 0) n = 0;
}

__device__ __forceinline__ float group16_max(float v) {
  for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float group16_sum(float v) {
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// rows [r0, r0 + nrows) x D of a row-major matrix (row stride ld, column offset c0) into an LDS
// tile of row stride LD; rows at or past `limit` are zero
__device__ __forceinline__ void load_tile(float* dst, int LD, int nrows, const float* src,
                                          int64_t ld, int64_t row0, int c0, int D, int r0,
                                          int limit) {
  for (int i = threadIdx.x; i < nrows * D; i += kThreads) {
    const int r = i / D, d = i - r * D;
    dst[r * LD + d] = (r0 + r < limit) ? src[(row0 + r0 + r) * ld + c0 + d] : 0.f;
  }
}

__global__ void __launch_bounds__(kThreads) k_attn_fwd(Args a, float* __restrict__ out,
                                                       float* __restrict__ lse) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int D = a.D, LD = D + 1, H = a.H;
  float* Qs = smem;           // [QB][LD]
  float* Ks = Qs + QB * LD;   // [KB][LD]
  float* Vs = Ks + KB * LD;   // [KB][LD]
  float* Ps = Vs + KB * LD;   // [QB][PLD]
  const int64_t g = blockIdx.x;
  const int h = blockIdx.y;
  const int tid = threadIdx.x, qr = tid >> 4, l16 = tid & 15;
  int64_t qo, ko;
  int nq, nk;
  segment(a.qptr, a.q_rows, g, qo, nq);
  segment(a.kptr, a.k_rows, g, ko, nk);
  const int64_t qi = a.q_shared ? 0 : qo;
  const int64_t HD = (int64_t)H * D;
  const float ninf = -__builtin_inff();

  for (int q0 = blockIdx.z * QB; q0 < nq; q0 += kSplit * QB) {
    __syncthreads();  // the previous query block's reads are done
    load_tile(Qs, LD, QB, a.q, a.ldq, qi, h * D, D, q0, nq);
    float m = ninf, l = 0.f;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    const bool qok = q0 + qr < nq;
    for (int k0 = 0; k0 < nk; k0 += KB) {
      __syncthreads();  // the previous key block's reads are done
      load_tile(Ks, LD, KB, a.k, a.ldk, ko, h * D, D, k0, nk);
      load_tile(Vs, LD, KB, a.v, a.ldv, ko, h * D, D, k0, nk);
      __syncthreads();
      float s[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int kk = l16 + 16 * i;
        float dot = 0.f;
        for (int d = 0; d < D; ++d) dot = fmaf(Qs[qr * LD + d], Ks[kk * LD + d], dot);
        s[i] = (k0 + kk < nk) ? dot * a.scale : ninf;
      }
      // key k0 of the block is always a real row, so the maximum is finite
      const float mnew = fmaxf(m, group16_max(fmaxf(s[0], s[1])));
      const float corr = expf(m - mnew);  // m = -inf on the first block: 0
      float rs = 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int kk = l16 + 16 * i;
        const bool ok = k0 + kk < nk;
        const float p = ok ? expf(s[i] - mnew) : 0.f;
        rs += p;
        float mv = 1.f;
        if (a.mask && ok && qok)
          mv = a.mask[a.moff[g] + ((int64_t)h * nq + (q0 + qr)) * nk + (k0 + kk)];
        Ps[qr * PLD + kk] = p * mv;
      }
      l = l * corr + group16_sum(rs);
      m = mnew;
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] *= corr;
#pragma unroll 2
      for (int kk = 0; kk < KB; ++kk) {
        const float p = Ps[qr * PLD + kk];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int d = l16 + 16 * j;
          if (d < D) acc[j] = fmaf(p, Vs[kk * LD + d], acc[j]);
        }
      }
    }
    if (qok) {
      const float inv = nk > 0 ? 1.f / l : 0.f;
      const int64_t row = qo + q0 + qr;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int d = l16 + 16 * j;
        if (d < D) out[row * HD + h * D + d] = acc[j] * inv;
      }
      if (l16 == 0) lse[row * H + h] = nk > 0 ? m + logf(l) : 0.f;
    }
  }
}

// the score-gradient tile of query block q0 x key block k0 into LDS: As = P * mask (written when
// As != nullptr), dSs = P * (dP * mask - delta) * scale; P recomputed from the saved log-sum-exp
__device__ __forceinline__ void score_grad_tile(const Args& a, int64_t g, int h, int nq, int nk,
                                                int q0, int k0, int LD, const float* Qs,
                                                const float* dOs, const float* Ks,
                                                const float* Vs, const float* lse_s,
                                                const float* del_s, float* As, float* dSs) {
  const int qr = threadIdx.x >> 4, l16 = threadIdx.x & 15, D = a.D;
  const bool qok = q0 + qr < nq;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int kk = l16 + 16 * i;
    float s = 0.f, dp = 0.f;
#pragma unroll 4
    for (int d = 0; d < D; ++d) {
      s = fmaf(Qs[qr * LD + d], Ks[kk * LD + d], s);
      dp = fmaf(dOs[qr * LD + d], Vs[kk * LD + d], dp);
    }
    const bool ok = qok && k0 + kk < nk;
    const float p = ok ? expf(s * a.scale - lse_s[qr]) : 0.f;
    float mv = 1.f;
    if (a.mask && ok) mv = a.mask[a.moff[g] + ((int64_t)h * nq + (q0 + qr)) * nk + (k0 + kk)];
    if (As) As[qr * PLD + kk] = p * mv;
    dSs[qr * PLD + kk] = p * (dp * mv - del_s[qr]) * a.scale;
  }
}

// query block q0's Q and dO rows into LDS, with each row's log-sum-exp and delta = <dO, O>
__device__ __forceinline__ void load_query_block(const Args& a, int h, int64_t qi, int64_t qo,
                                                 int nq, int q0, int LD, const float* out,
                                                 const float* dout, const float* lse, float* Qs,
                                                 float* dOs, float* lse_s, float* del_s) {
  const int qr = threadIdx.x >> 4, l16 = threadIdx.x & 15, D = a.D, H = a.H;
  const int64_t HD = (int64_t)H * D;
  load_tile(Qs, LD, QB, a.q, a.ldq, qi, h * D, D, q0, nq);
  load_tile(dOs, LD, QB, dout, HD, qo, h * D, D, q0, nq);
  const bool qok = q0 + qr < nq;
  const int64_t row = qo + q0 + qr;
  float t = 0.f;
  if (qok)
    for (int d = l16; d < D; d += 16)
      t = fmaf(dout[row * HD + h * D + d], out[row * HD + h * D + d], t);
  t = group16_sum(t);
  if (l16 == 0) {
    del_s[qr] = t;
    lse_s[qr] = qok ? lse[row * H + h] : 0.f;
  }
}

// dK, dV: workgroup z of a (set, head) owns key blocks z, z + kSplit, ...; a block's gradients
// stay in registers over all query blocks (fixed order) and are written once
__global__ void __launch_bounds__(kThreads)
    k_attn_bwd_dkv(Args a, const float* __restrict__ out, const float* __restrict__ dout,
                   const float* __restrict__ lse, float* __restrict__ dk, int64_t lddk,
                   float* __restrict__ dv, int64_t lddv) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int D = a.D, LD = D + 1;
  float* Qs = smem;             // [QB][LD]
  float* dOs = Qs + QB * LD;    // [QB][LD]
  float* Ks = dOs + QB * LD;    // [KB][LD]
  float* Vs = Ks + KB * LD;     // [KB][LD]
  float* As = Vs + KB * LD;     // [QB][PLD] the (dropped-out) probabilities
  float* dSs = As + QB * PLD;   // [QB][PLD] the score gradients, scaled
  float* lse_s = dSs + QB * PLD;  // [QB]
  float* del_s = lse_s + QB;      // [QB]
  const int64_t g = blockIdx.x;
  const int h = blockIdx.y;
  const int tid = threadIdx.x, kr = tid >> 3, l8 = tid & 7;
  int64_t qo, ko;
  int nq, nk;
  segment(a.qptr, a.q_rows, g, qo, nq);
  segment(a.kptr, a.k_rows, g, ko, nk);
  const int64_t qi = a.q_shared ? 0 : qo;

  for (int k0 = blockIdx.z * KB; k0 < nk; k0 += kSplit * KB) {
    __syncthreads();  // the previous key block's reads are done
    load_tile(Ks, LD, KB, a.k, a.ldk, ko, h * D, D, k0, nk);
    load_tile(Vs, LD, KB, a.v, a.ldv, ko, h * D, D, k0, nk);
    float dKa[16], dVa[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) dKa[j] = dVa[j] = 0.f;
    for (int q0 = 0; q0 < nq; q0 += QB) {
      __syncthreads();  // the previous query block's reads are done
      load_query_block(a, h, qi, qo, nq, q0, LD, out, dout, lse, Qs, dOs, lse_s, del_s);
      __syncthreads();
      score_grad_tile(a, g, h, nq, nk, q0, k0, LD, Qs, dOs, Ks, Vs, lse_s, del_s, As, dSs);
      __syncthreads();
#pragma unroll 1
      for (int qq = 0; qq < QB; ++qq) {
        const float pa = As[qq * PLD + kr], ps = dSs[qq * PLD + kr];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int d = l8 + 8 * j;
          if (d < D) {
            dVa[j] = fmaf(pa, dOs[qq * LD + d], dVa[j]);
            dKa[j] = fmaf(ps, Qs[qq * LD + d], dKa[j]);
          }
        }
      }
    }
    if (k0 + kr < nk) {
      const int64_t row = ko + k0 + kr;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int d = l8 + 8 * j;
        if (d < D) {
          dk[row * lddk + h * D + d] = dKa[j];
          dv[row * lddv + h * D + d] = dVa[j];
        }
      }
    }
  }
}

// dQ: workgroup z of a (set, head) owns query blocks z, z + kSplit, ...; a block's gradient stays
// in registers over all key blocks (fixed order) and is written once (zeros without keys)
__global__ void __launch_bounds__(kThreads)
    k_attn_bwd_dq(Args a, const float* __restrict__ out, const float* __restrict__ dout,
                  const float* __restrict__ lse, float* __restrict__ dq, int64_t lddq) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int D = a.D, LD = D + 1;
  float* Qs = smem;             // [QB][LD]
  float* dOs = Qs + QB * LD;    // [QB][LD]
  float* Ks = dOs + QB * LD;    // [KB][LD]
  float* Vs = Ks + KB * LD;     // [KB][LD]
  float* dSs = Vs + KB * LD;    // [QB][PLD]
  float* lse_s = dSs + QB * PLD;  // [QB]
  float* del_s = lse_s + QB;      // [QB]
  const int64_t g = blockIdx.x;
  const int h = blockIdx.y;
  const int tid = threadIdx.x, qr = tid >> 4, l16 = tid & 15;
  int64_t qo, ko;
  int nq, nk;
  segment(a.qptr, a.q_rows, g, qo, nq);
  segment(a.kptr, a.k_rows, g, ko, nk);
  const int64_t qi = a.q_shared ? 0 : qo;

  for (int q0 = blockIdx.z * QB; q0 < nq; q0 += kSplit * QB) {
    __syncthreads();  // the previous query block's reads are done
    load_query_block(a, h, qi, qo, nq, q0, LD, out, dout, lse, Qs, dOs, lse_s, del_s);
    float t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = 0.f;
    for (int k0 = 0; k0 < nk; k0 += KB) {
      __syncthreads();  // the previous key block's reads are done
      load_tile(Ks, LD, KB, a.k, a.ldk, ko, h * D, D, k0, nk);
      load_tile(Vs, LD, KB, a.v, a.ldv, ko, h * D, D, k0, nk);
      __syncthreads();
      score_grad_tile(a, g, h, nq, nk, q0, k0, LD, Qs, dOs, Ks, Vs, lse_s, del_s, nullptr, dSs);
      __syncthreads();
#pragma unroll 1
      for (int kk = 0; kk < KB; ++kk) {
        const float ps = dSs[qr * PLD + kk];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int d = l16 + 16 * j;
          if (d < D) t[j] = fmaf(ps, Ks[kk * LD + d], t[j]);
        }
      }
    }
    if (q0 + qr < nq) {
      const int64_t row = qo + q0 + qr;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int d = l16 + 16 * j;
        if (d < D) dq[row * lddq + h * D + d] = t[j];
      }
    }
  }
}

// mask_off[g] = heads * sum_{g' < g} nq_g' * nk_g' (one workgroup, tiles of kThreads sets)
__global__ void __launch_bounds__(kThreads)
    k_mask_offsets(const int32_t* __restrict__ qptr, int q_rows, const int32_t* __restrict__ kptr,
                   int k_rows, int64_t B, int H, int64_t* __restrict__ moff) {
  __shared__ int64_t s_wave[kThreads / 64];
  int64_t carry = 0;
  for (int64_t tile = 0; tile < B; tile += kThreads) {
    const int64_t g = tile + threadIdx.x;
    int64_t o, n = 0;
    if (g < B) {
      int nq, nk;
      segment(qptr, q_rows, g, o, nq);
      segment(kptr, k_rows, g, o, nk);
      n = (int64_t)H * nq * nk;
    }
    const int64_t at = block_exclusive_scan<kThreads>(n, carry, s_wave);
    if (g < B) moff[g] = at;
  }
  if (threadIdx.x == 0) moff[B] = carry;
}

// ---------------------------------------------------------------------------------------------
// y = LN(a + act(b)): one wave per row, the row in registers (C <= 512: 8 values per lane)
// ---------------------------------------------------------------------------------------------

constexpr int kMaxC = 512;
constexpr int kPerLane = kMaxC / 64;
constexpr int kRowsPerBlock = kThreads / 64;
constexpr int kMaxParts = 256;

__device__ __forceinline__ float act_f(float x, int act) {
  return act == LGNN_ACT_RELU ? fmaxf(x, 0.f) : x;
}

__global__ void __launch_bounds__(kThreads)
    k_res_norm_fwd(const float* __restrict__ a, int a_rows, const float* __restrict__ b, int act,
                   const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                   int64_t M, int C, float* __restrict__ y, float* __restrict__ mean,
                   float* __restrict__ rstd) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (row >= M) return;
  const int64_t arow = a_rows > 0 ? row % a_rows : row;
  float u[kPerLane];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < kPerLane; ++i) {
    const int c = lane + 64 * i;
    u[i] = 0.f;
    if (c < C) {
      u[i] = (a ? a[arow * C + c] : 0.f) + act_f(b[row * C + c], act);
      s += u[i];
    }
  }
  if (!gamma) {
#pragma unroll
    for (int i = 0; i < kPerLane; ++i) {
      const int c = lane + 64 * i;
      if (c < C) y[row * C + c] = u[i];
    }
    return;
  }
  const float mu = wave_sum(s) / (float)C;
  float v = 0.f;
#pragma unroll
  for (int i = 0; i < kPerLane; ++i) {
    const int c = lane + 64 * i;
    if (c < C) v = fmaf(u[i] - mu, u[i] - mu, v);
  }
  const float rs = 1.f / sqrtf(wave_sum(v) / (float)C + eps);  // biased variance
#pragma unroll
  for (int i = 0; i < kPerLane; ++i) {
    const int c = lane + 64 * i;
    if (c < C) y[row * C + c] = fmaf((u[i] - mu) * rs, gamma[c], beta[c]);
  }
  if (lane == 0) {
    mean[row] = mu;
    rstd[row] = rs;
  }
}

// Workgroup p owns rows [p * rows_per, (p + 1) * rows_per), its wave w every fourth of them: the
// column sums (dgamma, dbeta) of a workgroup's rows are added in that fixed order, then the four
// waves' in wave order, into part[0][p][C] (dgamma) and part[1][p][C] (dbeta);
// lgnn_reduce_partials sums the workgroups.
__global__ void __launch_bounds__(kThreads)
    k_res_norm_bwd(const float* __restrict__ a, int a_rows, const float* __restrict__ b, int act,
                   const float* __restrict__ gamma, int64_t M, int C,
                   const float* __restrict__ mean, const float* __restrict__ rstd,
                   const float* __restrict__ dy, float* __restrict__ da, float* __restrict__ db,
                   float* __restrict__ part, int64_t rows_per) {
  __shared__ float red[kRowsPerBlock][2][kMaxC];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per;
  const int64_t r1 = r0 + rows_per < M ? r0 + rows_per : M;
  float dg[kPerLane], dbt[kPerLane];
#pragma unroll
  for (int i = 0; i < kPerLane; ++i) dg[i] = dbt[i] = 0.f;
  for (int64_t row = r0 + w; row < r1; row += kRowsPerBlock) {
    const int64_t arow = a_rows > 0 ? row % a_rows : row;
    float g[kPerLane], xh[kPerLane], bv[kPerLane];
    float s1 = 0.f, s2 = 0.f;
    const float mu = gamma ? mean[row] : 0.f, rs = gamma ? rstd[row] : 1.f;
#pragma unroll
    for (int i = 0; i < kPerLane; ++i) {
      const int c = lane + 64 * i;
      g[i] = xh[i] = bv[i] = 0.f;
      if (c < C) {
        const float d = dy[row * C + c];
        bv[i] = b[row * C + c];
        if (gamma) {
          const float u = (a ? a[arow * C + c] : 0.f) + act_f(bv[i], act);
          xh[i] = (u - mu) * rs;
          g[i] = d * gamma[c];
          s1 += g[i];
          s2 = fmaf(g[i], xh[i], s2);
          dg[i] = fmaf(d, xh[i], dg[i]);
          dbt[i] += d;
        } else {
          g[i] = d;
        }
      }
    }
    if (gamma) {
      s1 = wave_sum(s1) / (float)C;
      s2 = wave_sum(s2) / (float)C;
    }
#pragma unroll
    for (int i = 0; i < kPerLane; ++i) {
      const int c = lane + 64 * i;
      if (c < C) {
        const float du = gamma ? rs * (g[i] - s1 - xh[i] * s2) : g[i];
        if (da) da[row * C + c] = du;
        if (db) db[row * C + c] = (act == LGNN_ACT_RELU && !(bv[i] > 0.f)) ? 0.f : du;
      }
    }
  }
  if (!part) return;
#pragma unroll
  for (int i = 0; i < kPerLane; ++i) {
    const int c = lane + 64 * i;
    if (c < C) {
      red[w][0][c] = dg[i];
      red[w][1][c] = dbt[i];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += kThreads) {
    const int k = i / C, c = i - k * C;
    float t = red[0][k][c];
    for (int ww = 1; ww < kRowsPerBlock; ++ww) t += red[ww][k][c];
    part[((int64_t)k * gridDim.x + blockIdx.x) * C + c] = t;
  }
}

// ---------------------------------------------------------------------------------------------
// readout of [B * S, C] rows: the mean over a set's S rows (or the rows as they are), a set with
// no input row (gptr given and empty) zero: what nan_to_num leaves of PyG's all-masked softmax
// ---------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kThreads)
    k_readout_fwd(const float* __restrict__ x, const int32_t* __restrict__ gptr, int64_t n, int S,
                  int C, int mean, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t per = mean ? C : (int64_t)S * C;
  const int64_t g = i / per;
  float r = 0.f;
  if (!gptr || gptr[g + 1] > gptr[g]) {
    if (mean) {
      const int c = (int)(i - g * per);
      for (int s = 0; s < S; ++s) r += x[(g * S + s) * C + c];
      r /= (float)S;
    } else {
      r = x[i];
    }
  }
  out[i] = r;
}

__global__ void __launch_bounds__(kThreads)
    k_readout_bwd(const float* __restrict__ dout, const int32_t* __restrict__ gptr, int64_t n,
                  int S, int C, int mean, float* __restrict__ dx) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t g = i / ((int64_t)S * C);
  float r = 0.f;
  if (!gptr || gptr[g + 1] > gptr[g]) r = mean ? dout[g * C + i % C] / (float)S : dout[i];
  dx[i] = r;
}

// y = a + b (the two gradient paths that meet at a block's input; y may alias a or b)
__global__ void __launch_bounds__(kThreads)
    k_add(const float* a, const float* b, float* y, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) y[i] = a[i] + b[i];
}

static bool attn_shape_ok(int64_t B, int H, int D, int q_rows, int q_shared, int k_rows,
                          const void* qptr, const void* kptr) {
  if (B < 0 || B > 2147483647LL || H < 1 || D < 1 || D > LGNN_SET_ATTN_MAX_D) return false;
  if ((int64_t)H * D > LGNN_SET_ATTN_MAX_HD) return false;
  if (!qptr && q_rows < 0) return false;
  if (!kptr && k_rows < 0) return false;
  if (q_shared && qptr) return false;
  return true;
}

static Args make_args(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v,
                      int64_t ldv, const int32_t* qptr, int q_rows, int q_shared,
                      const int32_t* kptr, int k_rows, int H, int D, const float* mask,
                      const int64_t* moff) {
  Args a;
  a.q = q; a.k = k; a.v = v;
  a.ldq = ldq; a.ldk = ldk; a.ldv = ldv;
  a.qptr = qptr; a.kptr = kptr;
  a.q_rows = q_rows; a.q_shared = q_shared; a.k_rows = k_rows;
  a.H = H; a.D = D;
  a.scale = 1.f / sqrtf((float)D);
  a.mask = mask; a.moff = moff;
  return a;
}

}  // namespace lgnn_setattn

using namespace lgnn_setattn;

extern "C" int lgnn_set_attn_mask_offsets(const int32_t* qptr, int q_rows, const int32_t* kptr,
                                          int k_rows, int64_t num_sets, int heads,
                                          int64_t* mask_off, void* stream) {
  if (num_sets < 0 || heads < 1 || !mask_off || (!qptr && q_rows < 0) || (!kptr && k_rows < 0))
    return LGNN_EINVAL;
  return launch(k_mask_offsets, dim3(1), dim3(kThreads), as_stream(stream), qptr, q_rows, kptr,
                k_rows, num_sets, heads, mask_off);
}

extern "C" int lgnn_set_attn_fwd(const float* q, int64_t ldq, const float* k, int64_t ldk,
                                 const float* v, int64_t ldv, const int32_t* qptr, int q_rows,
                                 int q_shared, const int32_t* kptr, int k_rows, int64_t num_sets,
                                 int heads, int head_dim, const float* mask,
                                 const int64_t* mask_off, float* out, float* lse, void* stream) {
  if (!attn_shape_ok(num_sets, heads, head_dim, q_rows, q_shared, k_rows, qptr, kptr))
    return LGNN_EINVAL;
  if ((mask != nullptr) != (mask_off != nullptr)) return LGNN_EINVAL;
  if (num_sets == 0) return LGNN_OK;
  const Args a = make_args(q, ldq, k, ldk, v, ldv, qptr, q_rows, q_shared, kptr, k_rows, heads,
                           head_dim, mask, mask_off);
  const size_t lds = ((size_t)(QB + 2 * KB) * (head_dim + 1) + QB * PLD) * sizeof(float);
  return launch_lds(k_attn_fwd, dim3((unsigned)num_sets, heads, kSplit), dim3(kThreads), lds,
                    as_stream(stream), a, out, lse);
}

extern "C" int lgnn_set_attn_bwd(const float* q, int64_t ldq, const float* k, int64_t ldk,
                                 const float* v, int64_t ldv, const int32_t* qptr, int q_rows,
                                 int q_shared, const int32_t* kptr, int k_rows, int64_t num_sets,
                                 int heads, int head_dim, const float* mask,
                                 const int64_t* mask_off, const float* out, const float* dout,
                                 const float* lse, float* dq, int64_t lddq, float* dk,
                                 int64_t lddk, float* dv, int64_t lddv, void* stream) {
  if (!attn_shape_ok(num_sets, heads, head_dim, q_rows, q_shared, k_rows, qptr, kptr))
    return LGNN_EINVAL;
  if ((mask != nullptr) != (mask_off != nullptr)) return LGNN_EINVAL;
  if (num_sets == 0) return LGNN_OK;
  const Args a = make_args(q, ldq, k, ldk, v, ldv, qptr, q_rows, q_shared, kptr, k_rows, heads,
                           head_dim, mask, mask_off);
  const size_t lds =
      ((size_t)(2 * QB + 2 * KB) * (head_dim + 1) + 2 * QB * PLD + 2 * QB) * sizeof(float);
  const dim3 grid((unsigned)num_sets, heads, kSplit);
  if (const int e = launch_lds(k_attn_bwd_dkv, grid, dim3(kThreads), lds, as_stream(stream), a, out,
                               dout, lse, dk, lddk, dv, lddv)) return e;
  return launch_lds(k_attn_bwd_dq, grid, dim3(kThreads), lds - QB * PLD * sizeof(float),
                    as_stream(stream), a, out, dout, lse, dq, lddq);
}

extern "C" int lgnn_res_norm_fwd(const float* a, int a_rows, const float* b, int act,
                                 const float* gamma, const float* beta, float eps, int64_t M,
                                 int C, float* y, float* mean, float* rstd, void* stream) {
  if (M < 0 || M > 2147483647LL || C < 1 || C > kMaxC || a_rows < 0 ||
      (act != LGNN_ACT_NONE && act != LGNN_ACT_RELU))
    return LGNN_EINVAL;
  if ((gamma != nullptr) != (beta != nullptr)) return LGNN_EINVAL;
  if (M == 0) return LGNN_OK;
  if (gamma && (!mean || !rstd)) return LGNN_EINVAL;
  if (a_rows > 0 && !a) return LGNN_EINVAL;
  if (!b || !y) return LGNN_EINVAL;
  const unsigned grid = (unsigned)((M + kRowsPerBlock - 1) / kRowsPerBlock);
  return launch(k_res_norm_fwd, dim3(grid), dim3(kThreads), as_stream(stream), a, a_rows, b, act,
                gamma, beta, eps, M, C, y, mean, rstd);
}

extern "C" int lgnn_res_norm_bwd_partials(int64_t M) {
  if (M <= 0) return 1;
  const int64_t blocks = (M + kRowsPerBlock - 1) / kRowsPerBlock;
  return (int)(blocks < kMaxParts ? blocks : kMaxParts);
}

extern "C" int lgnn_res_norm_bwd(const float* a, int a_rows, const float* b, int act,
                                 const float* gamma, int64_t M, int C, const float* mean,
                                 const float* rstd, const float* dy, float* da, float* db,
                                 float* part, int num_partials, void* stream) {
  if (M < 0 || M > 2147483647LL || C < 1 || C > kMaxC || a_rows < 0 ||
      (act != LGNN_ACT_NONE && act != LGNN_ACT_RELU))
    return LGNN_EINVAL;
  if (num_partials != lgnn_res_norm_bwd_partials(M)) return LGNN_EINVAL;
  if (gamma && !part) return LGNN_EINVAL;
  if (M > 0 && ((gamma && (!mean || !rstd)) || (a_rows > 0 && !a))) return LGNN_EINVAL;
  if (M == 0) {  // no row: the column sums are zero
    if (part) {
      hipError_t e = hipMemsetAsync(part, 0, sizeof(float) * 2 * C, as_stream(stream));
      if (e != hipSuccess) return (int)e;
    }
    return LGNN_OK;
  }
  if (!b || !dy) return LGNN_EINVAL;
  const int64_t rows_per = (M + num_partials - 1) / num_partials;
  return launch(k_res_norm_bwd, dim3(num_partials), dim3(kThreads), as_stream(stream), a, a_rows, b,
                act, gamma, M, C, mean, rstd, dy, da, db, gamma ? part : nullptr, rows_per);
}

extern "C" int lgnn_set_readout_fwd(const float* x, const int32_t* gptr, int64_t num_sets,
                                    int rows, int C, int mean, float* out, void* stream) {
  if (num_sets < 0 || rows < 1 || C < 1) return LGNN_EINVAL;
  const int64_t n = num_sets * (mean ? (int64_t)C : (int64_t)rows * C);
  if (n == 0) return LGNN_OK;
  if (!x || !out || n > 2147483647LL * kThreads) return LGNN_EINVAL;
  return launch(k_readout_fwd, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads),
                as_stream(stream), x, gptr, n, rows, C, mean, out);
}

extern "C" int lgnn_set_readout_bwd(const float* dout, const int32_t* gptr, int64_t num_sets,
                                    int rows, int C, int mean, float* dx, void* stream) {
  if (num_sets < 0 || rows < 1 || C < 1) return LGNN_EINVAL;
  const int64_t n = num_sets * rows * C;
  if (n == 0) return LGNN_OK;
  if (!dout || !dx || n > 2147483647LL * kThreads) return LGNN_EINVAL;
  return launch(k_readout_bwd, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads),
                as_stream(stream), dout, gptr, n, rows, C, mean, dx);
}

extern "C" int lgnn_add(const float* a, const float* b, float* y, int64_t n, void* stream) {
  if (n < 0 || n > 2147483647LL * kThreads) return LGNN_EINVAL;
  if (n == 0) return LGNN_OK;
  if (!a || !b || !y) return LGNN_EINVAL;
  return launch(k_add, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads),
                as_stream(stream), a, b, y, n);
}
