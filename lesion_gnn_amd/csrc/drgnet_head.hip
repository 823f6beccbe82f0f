// DRGNet head for gfx950: Conv1d(1, c0, D, stride D) -> ELU -> MaxPool1d(2, 2) -> Conv1d(c0, c1, 5)
// -> ELU -> flatten -> Lin(dense, H) -> ELU -> dropout mask -> Lin(H, C), forward in one launch and
// backward in three. Reference: src/lesion_gnn/models/drgnet.py:38-48 (the modules), :60-64 (the
// calls). Replaces the MIOpen convolutions, hipBLAS linears and elementwise launches torch ran.
//
//   x [B, k*D] (row r of graph b at x[b, r*D .. (r+1)*D), rows past the graph's size zero)
//   z1[b,r,:]  = W1 x_row + b1                                   K2 = k / 2, P = K2 - 4
//   a1[b,q,:]  = max(ELU(z1[b,2q,:]), ELU(z1[b,2q+1,:]))         ties: the first of the pair
//   a2[b,c,p]  = ELU(b2[c] + sum_{i,t} W2[c,i,t] a1[b,p+t,i])    flattened c * P + p
//   h          = ELU(L0 a2 + b0) * mask,  logits = L1 h + bL1
//
// A workgroup takes passes of gb <= 4 graphs (grid-stride; gb = 1 until B fills four workgroups
// per CU), so every weight it reads serves gb graphs; a1, a2 and h of the pass live in LDS, and
// conv2's weights too when they fit.
//  forward  k_head_fwd: conv1 as 16-row x 16-channel tiles, one wave per tile, D streamed in
//           64-column chunks through a wave-private LDS stage (rows and weights, coalesced); the
//           tile product is mfma_f32_16x16x4f32 when c0 % 16 == 0 and the same lane map on FMAs
//           otherwise. A lane holds both rows of a pooled pair, so ELU + max pool run in registers
//           and the choice leaves as one bit per (b, q, i) (a wave ballot). conv2: one thread per
//           output from LDS. Lin0: a wave per two output rows, lanes over dense, gb accumulators (gb <
//           16 rows never fill an MFMA tile: FMAs). Saved for the backward: a1, the bits, a2, h
//           before the mask.
//  backward k_head_bwd (same passes): dL1 / dbL1, dh = (L1^T dlogits) mask ELU'(h) -> global [B, He];
//           da2 = L0^T dh (thread per column, L0 read once per pass); dW2 / db2; da1 -> dz1 of the
//           chosen row (in place of a1 in LDS); then one thread per column d forms dW1[:, d] and
//           dx[:, d] from the chosen rows (the bits), D streamed with nothing resident.
//           Every small parameter gradient is owned per element by one thread of the workgroup,
//           which adds it across passes into the workgroup's own slab: no atomics, a fixed order.
//           Then lgnn_s3_wgrad (dL0 = dh^T a2 and db0, split over B in fixed chunks) and one
//           lgnn_reduce_partials_multi over the eight slabs.
// Bound: launch / latency at the reference shape (120 k MAC per graph); Lin0's weights (H * dense
// floats from L2 per pass) are the largest stream.
#include <algorithm>

#include "launch.h"
#include "wg.h"

namespace lgnn_drgnet_head {

constexpr int NT = 256;
constexpr int NW = NT / 64;
constexpr int GBMAX = 4;                    // graphs of one pass
constexpr int DC = 64;                      // conv1: columns of one chunk (one per lane)
constexpr int DCP = DC + 1;                 // its LDS row pitch
constexpr int STAGE = NW * 2 * 16 * DCP;    // floats: per wave 16 rows of x and 16 of W1
constexpr int KT = 5;                       // conv2 taps (reference drgnet.py:40)
constexpr int MAXC = 16;                    // classes
constexpr int QB = 4;                       // conv1 backward: pooled pairs loaded ahead
constexpr int W2LDS = 4096;                 // floats of conv2 weights a workgroup copies to LDS
constexpr size_t kPlainLds = 64 * 1024;
constexpr size_t kMaxLds = 160 * 1024;
constexpr int64_t kSlabBudget = (int64_t)16 << 20;  // floats of per-workgroup slabs
constexpr int kMaxSlots = 512;

struct Dims {
  int64_t B;
  int k, D, c0, c1, H, C;
  int K2, P, dense, He, a1s, nct, gb;
  int w2off;  // floats: where conv2's weights sit in LDS, or -1 (too large: read from global)
};

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// conv2's weights for this workgroup: a copy in LDS when the plan left room, else as they are
__device__ __forceinline__ const float* stage_w2(const Dims& dm, const float* W2, float* lds) {
  if (dm.w2off < 0) return W2;
  for (int e = threadIdx.x; e < dm.c1 * dm.c0 * KT; e += NT) lds[e] = W2[e];
  __syncthreads();
  return lds;
}

// add v into the workgroup's slab element (owned by this thread); the first pass stores
__device__ __forceinline__ void slab_add(float* p, float v, bool first) { *p = first ? v : *p + v; }

template <bool kMfma>
__global__ void __launch_bounds__(NT)
    k_head_fwd(Dims dm, const float* __restrict__ x, const float* __restrict__ W1,
               const float* __restrict__ b1, const float* __restrict__ W2,
               const float* __restrict__ b2, const float* __restrict__ L0,
               const float* __restrict__ b0v, const float* __restrict__ L1,
               const float* __restrict__ bL1, const float* __restrict__ mask,
               float* __restrict__ logits, float* __restrict__ a1o, uint16_t* __restrict__ selo,
               float* __restrict__ a2o, float* __restrict__ ho) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int k = dm.k, D = dm.D, c0 = dm.c0, H = dm.H, C = dm.C;
  const int K2 = dm.K2, P = dm.P, dense = dm.dense, a1s = dm.a1s, nct = dm.nct, gb = dm.gb;
  float* s_a1 = smem;                      // [gb][K2][a1s]
  float* s_u = smem + gb * K2 * a1s;       // the conv1 stage, then a2 [gb][dense] and h [gb][H]
  float* s_a2 = s_u;
  float* s_h = s_u + gb * dense;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* w2 = stage_w2(dm, W2, smem + dm.w2off);
  const int R1 = 2 * K2;  // rows of a graph that reach the pool (an odd k drops its last)
  const int64_t npass = (dm.B + gb - 1) / gb;

  for (int64_t pass = blockIdx.x; pass < npass; pass += gridDim.x) {
    const int64_t g0 = pass * gb;
    const int gbc = (int)min((int64_t)gb, dm.B - g0);
    // ---- conv1 + ELU + max pool: tiles of 16 rows x 16 channels over the pass's rows
    const int R = gbc * R1, nrt = (R + 15) / 16, ntiles = nrt * nct;
    float* xs = s_u + wave * (2 * 16 * DCP);
    float* ws = xs + 16 * DCP;
    for (int t0 = 0; t0 < ntiles; t0 += NW) {
      const int t = t0 + wave;
      const bool act = t < ntiles;
      const int rt = act ? t / nct : 0, ct = act ? t % nct : 0;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int d0 = 0; d0 < D; d0 += DC) {
        __syncthreads();  // the stage's previous readers are done
        const int d = d0 + lane;
        const bool dok = act && d < D;
        const int dcl = dok ? d : 0;
        // all 32 loads of the chunk in flight (clamped addresses, selected after)
        float xv[16], wv[16];
        int g = rt * 16 / R1, r = rt * 16 - g * R1;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
          const bool okx = dok && rt * 16 + rr < R, okw = dok && ct * 16 + rr < c0;
          const float vx = x[((g0 + (okx ? g : 0)) * k + (okx ? r : 0)) * (int64_t)D + dcl];
          const float vw = W1[(int64_t)(okw ? ct * 16 + rr : 0) * D + dcl];
          xv[rr] = okx ? vx : 0.f;
          wv[rr] = okw ? vw : 0.f;
          if (++r == R1) {
            r = 0;
            ++g;
          }
        }
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
          xs[rr * DCP + lane] = xv[rr];
          ws[rr * DCP + lane] = wv[rr];
        }
        __syncthreads();
        if (kMfma) {
          // A[i = lane & 15][kk = lane >> 4] = x row i, B[kk][j = lane & 15] = W1 channel j
          const int o = (lane & 15) * DCP + (lane >> 4);
#pragma unroll 4
          for (int dd = 0; dd < DC; dd += 4) acc = mfma16(xs[o + dd], ws[o + dd], acc);
        } else {
          const int ro = (lane >> 4) * 4 * DCP, wo = (lane & 15) * DCP;
#pragma unroll 4
          for (int dd = 0; dd < DC; ++dd) {
            const float wv = ws[wo + dd];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(xs[ro + e * DCP + dd], wv, acc[e]);
          }
        }
      }
      if (act) {  // acc[e] = z1[row rt*16 + (lane >> 4)*4 + e][channel ct*16 + (lane & 15)]
        const int ch = ct * 16 + (lane & 15);
        const float bias = ch < c0 ? b1[ch] : 0.f;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int row = rt * 16 + (lane >> 4) * 4 + 2 * j;  // even: the pair (row, row + 1)
          const float e0 = elu_f(acc[2 * j] + bias), e1 = elu_f(acc[2 * j + 1] + bias);
          const bool second = e1 > e0;  // a tie keeps the first (torch max_pool1d)
          const bool valid = row < R && ch < c0;
          const unsigned long long bal = __ballot(valid && second);
          if (row < R) {
            const int g = row / R1, q = (row - g * R1) >> 1;
            if (valid) {
              const float a = second ? e1 : e0;
              s_a1[(g * K2 + q) * a1s + ch] = a;
              a1o[((g0 + g) * K2 + q) * (int64_t)c0 + ch] = a;
            }
            if ((lane & 15) == 0)
              selo[((g0 + g) * K2 + q) * (int64_t)nct + ct] =
                  (uint16_t)((bal >> (16 * (lane >> 4))) & 0xffffull);
          }
        }
      }
    }
    __syncthreads();
    // the pass's dropout multipliers (1 without a mask) into h's place: Lin0's lane 0 then reads
    // LDS instead of waiting on one global load per output
    for (int e = tid; e < gbc * H; e += NT) s_h[e] = mask ? mask[g0 * H + e] : 1.f;
    // ---- conv2 + ELU: one thread per output (g, c, p)
    for (int e = tid; e < gbc * dense; e += NT) {
      const int g = e / dense, m = e - g * dense, c = m / P, p = m - c * P;
      float acc = b2[c];
      const float* w = w2 + c * c0 * KT;
      const float* a = s_a1 + (g * K2 + p) * a1s;
#pragma unroll 4
      for (int i = 0; i < c0; ++i)
#pragma unroll
        for (int t = 0; t < KT; ++t) acc = fmaf(w[i * KT + t], a[t * a1s + i], acc);
      acc = elu_f(acc);
      s_a2[e] = acc;
      a2o[(g0 + g) * (int64_t)dense + m] = acc;
    }
    __syncthreads();
    // ---- Lin0 + ELU + mask: one wave per output row j, lanes over dense
    for (int j0 = 2 * wave; j0 < H; j0 += 2 * NW) {
      float acc[2][GBMAX];
#pragma unroll
      for (int g = 0; g < GBMAX; ++g) acc[0][g] = acc[1][g] = 0.f;
      const int j1 = j0 + 1 < H ? j0 + 1 : j0;  // an odd H: the last row twice, stored once
      const float bja = b0v[j0], bjb = b0v[j1];
      const float* wa = L0 + (int64_t)j0 * dense;
      const float* wb = L0 + (int64_t)j1 * dense;
      for (int m0 = 0; m0 < dense; m0 += 64 * 8) {
        float va[8], vb[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {  // sixteen loads in flight
          const int m = m0 + 64 * u + lane, mc = m < dense ? m : dense - 1;
          va[u] = wa[mc];
          vb[u] = wb[mc];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int m = m0 + 64 * u + lane;
          if (m < dense) {
#pragma unroll
            for (int g = 0; g < GBMAX; ++g)
              if (g < gbc) {
                const float av = s_a2[g * dense + m];
                acc[0][g] = fmaf(va[u], av, acc[0][g]);
                acc[1][g] = fmaf(vb[u], av, acc[1][g]);
              }
          }
        }
      }
      // the 2 * GBMAX lane sums side by side: each xor step's shuffles are independent
      for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
          for (int g = 0; g < GBMAX; ++g) acc[jj][g] += __shfl_xor(acc[jj][g], o, 64);
      }
      if (lane == 0) {
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          const int j = j0 + jj;
#pragma unroll
          for (int g = 0; g < GBMAX; ++g) {
            if (g < gbc && j < H) {
              const float hv = elu_f(acc[jj][g] + (jj ? bjb : bja));
              ho[(g0 + g) * (int64_t)H + j] = hv;
              s_h[g * H + j] *= hv;
            }
          }
        }
      }
    }
    __syncthreads();
    // ---- Lin1: one wave per logit
    for (int o = wave; o < gbc * C; o += NW) {
      const int g = o / C, c = o - g * C;
      float s = 0.f;
      for (int j = lane; j < H; j += 64) s = fmaf(L1[c * H + j], s_h[g * H + j], s);
      s = wave_sum(s);
      if (lane == 0) logits[(g0 + g) * (int64_t)C + c] = s + bL1[c];
    }
    __syncthreads();  // h shares LDS with the next pass's stage
  }
}

struct Slabs {  // this launch's per-workgroup partial sums, [slots][len] each
  float *dW1, *db1, *dW2, *db2, *dL1, *dbL1;
};

__global__ void __launch_bounds__(NT)
    k_head_bwd(Dims dm, const float* __restrict__ dlog, const float* __restrict__ x,
               const float* __restrict__ W1, const float* __restrict__ W2,
               const float* __restrict__ L0, const float* __restrict__ L1,
               const float* __restrict__ mask, const float* __restrict__ a1i,
               const uint16_t* __restrict__ seli, const float* __restrict__ a2i,
               const float* __restrict__ hi, float* __restrict__ dx, float* __restrict__ dh,
               Slabs sl) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int k = dm.k, D = dm.D, c0 = dm.c0, c1 = dm.c1, H = dm.H, C = dm.C, He = dm.He;
  const int K2 = dm.K2, P = dm.P, dense = dm.dense, a1s = dm.a1s, nct = dm.nct, gb = dm.gb;
  float* s_a1 = smem;                    // [gb][K2][a1s]: a1, then dz1 of the chosen rows
  float* s_dz2 = s_a1 + gb * K2 * a1s;   // [gb][dense]
  float* s_hm = s_dz2 + gb * dense;      // [gb][H]: h * mask
  float* s_dh = s_hm + gb * H;           // [gb][H]
  float* s_dl = s_dh + gb * H;           // [gb][C]
  const int tid = threadIdx.x;
  const float* w2 = stage_w2(dm, W2, smem + dm.w2off);
  const int64_t npass = (dm.B + gb - 1) / gb;
  const int64_t slot = blockIdx.x;
  float* const dW1 = sl.dW1 + slot * c0 * (int64_t)D;
  float* const db1 = sl.db1 + slot * c0;
  float* const dW2 = sl.dW2 + slot * (int64_t)(c1 * c0 * KT);
  float* const db2 = sl.db2 + slot * c1;
  float* const dL1 = sl.dL1 + slot * (int64_t)(C * H);
  float* const dbL1 = sl.dbL1 + slot * C;

  for (int64_t pass = blockIdx.x; pass < npass; pass += gridDim.x) {
    const bool first = pass == (int64_t)blockIdx.x;
    const int64_t g0 = pass * gb;
    const int gbc = (int)min((int64_t)gb, dm.B - g0);
    __syncthreads();
    for (int e = tid; e < gbc * C; e += NT) s_dl[e] = dlog[g0 * C + e];
    for (int e = tid; e < gbc * H; e += NT) {
      const int64_t o = g0 * H + e;
      s_hm[e] = mask ? hi[o] * mask[o] : hi[o];
    }
    __syncthreads();
    // ---- Lin1 backward: dL1, dbL1, dh = (L1^T dlogits) * mask * ELU'(h)
    for (int e = tid; e < C * H; e += NT) {
      const int c = e / H, j = e - c * H;
      float s = 0.f;
      for (int g = 0; g < gbc; ++g) s = fmaf(s_dl[g * C + c], s_hm[g * H + j], s);
      slab_add(dL1 + e, s, first);
    }
    if (tid < C) {
      float s = 0.f;
      for (int g = 0; g < gbc; ++g) s += s_dl[g * C + tid];
      slab_add(dbL1 + tid, s, first);
    }
    for (int e = tid; e < gbc * H; e += NT) {
      const int g = e / H, j = e - g * H;
      float s = 0.f;
      for (int c = 0; c < C; ++c) s = fmaf(s_dl[g * C + c], L1[c * H + j], s);
      const int64_t o = g0 * H + e;
      const float v = s * (mask ? mask[o] : 1.f) * elu_grad_from_out(hi[o]);
      s_dh[e] = v;
      dh[(g0 + g) * (int64_t)He + j] = v;
      if (j == 0 && He != H) dh[(g0 + g) * (int64_t)He + H] = 0.f;  // the pad column
    }
    for (int e = tid; e < gbc * K2 * c0; e += NT) {
      const int gq = e / c0, i = e - gq * c0;
      s_a1[gq * a1s + i] = a1i[g0 * K2 * c0 + e];
    }
    __syncthreads();
    // ---- Lin0 backward to its input: da2 = L0^T dh, dz2 = da2 * ELU'(a2); thread per column
    for (int m = tid; m < dense; m += NT) {
      float acc[GBMAX];
#pragma unroll
      for (int g = 0; g < GBMAX; ++g) acc[g] = 0.f;
      for (int j0 = 0; j0 < H; j0 += 8) {
        float wv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)  // eight loads in flight
          wv[u] = L0[(int64_t)(j0 + u < H ? j0 + u : H - 1) * dense + m];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          if (j0 + u < H) {
#pragma unroll
            for (int g = 0; g < GBMAX; ++g)
              if (g < gbc) acc[g] = fmaf(wv[u], s_dh[g * H + j0 + u], acc[g]);
          }
        }
      }
#pragma unroll
      for (int g = 0; g < GBMAX; ++g)
        if (g < gbc)
          s_dz2[g * dense + m] = acc[g] * elu_grad_from_out(a2i[(g0 + g) * (int64_t)dense + m]);
    }
    __syncthreads();
    // ---- conv2 backward: dW2, db2 (a1 still in LDS)
    for (int e = tid; e < c1 * c0 * KT; e += NT) {
      const int c = e / (c0 * KT), rem = e - c * (c0 * KT), i = rem / KT, t = rem - i * KT;
      float s = 0.f;
      for (int g = 0; g < gbc; ++g) {
        const float* z = s_dz2 + g * dense + c * P;
        const float* a = s_a1 + (g * K2 + t) * a1s + i;
#pragma unroll 4
        for (int p = 0; p < P; ++p) s = fmaf(z[p], a[p * a1s], s);
      }
      slab_add(dW2 + e, s, first);
    }
    if (tid < c1) {
      float s = 0.f;
      for (int g = 0; g < gbc; ++g)
        for (int p = 0; p < P; ++p) s += s_dz2[g * dense + tid * P + p];
      slab_add(db2 + tid, s, first);
    }
    __syncthreads();
    // ---- da1 -> dz1 of the chosen row of each pair, in place of a1 (each thread its own element)
    for (int e = tid; e < gbc * K2 * c0; e += NT) {
      const int gq = e / c0, i = e - gq * c0, g = gq / K2, q = gq - g * K2;
      float s = 0.f;
#pragma unroll 4
      for (int c = 0; c < c1; ++c) {
        const float* w = w2 + (c * c0 + i) * KT;
        const float* z = s_dz2 + g * dense + c * P;
#pragma unroll
        for (int t = 0; t < KT; ++t) {
          const int p = q - t;
          if (p >= 0 && p < P) s = fmaf(w[t], z[p], s);
        }
      }
      s_a1[gq * a1s + i] = s * elu_grad_from_out(s_a1[gq * a1s + i]);
    }
    __syncthreads();
    if (tid < c0) {
      float s = 0.f;
      for (int gq = 0; gq < gbc * K2; ++gq) s += s_a1[gq * a1s + tid];
      slab_add(db1 + tid, s, first);
    }
    // ---- conv1 backward: thread d owns column d of dW1 and of every dx row
    for (int d = tid; d < D; d += NT) {
      for (int ct = 0; ct < nct; ++ct) {
        float w[16], acc[16];
#pragma unroll
        for (int ii = 0; ii < 16; ++ii) {
          const int ch = ct * 16 + ii;
          w[ii] = ch < c0 ? W1[(int64_t)ch * D + d] : 0.f;
          acc[ii] = 0.f;
        }
        for (int g = 0; g < gbc; ++g) {
          const float* xg = x + (g0 + g) * (int64_t)k * D + d;
          float* dxg = dx + (g0 + g) * (int64_t)k * D + d;
          for (int q0 = 0; q0 < K2; q0 += QB) {
            float x0[QB], x1[QB];
            unsigned bits[QB];
#pragma unroll
            for (int u = 0; u < QB; ++u) {  // the block's loads in flight
              const int q = q0 + u < K2 ? q0 + u : K2 - 1;
              x0[u] = xg[(int64_t)(2 * q) * D];
              x1[u] = xg[(int64_t)(2 * q + 1) * D];
              bits[u] = seli[((g0 + g) * K2 + q) * (int64_t)nct + ct];
            }
#pragma unroll
            for (int u = 0; u < QB; ++u) {
              const int q = q0 + u;
              if (q < K2) {
                const float* z = s_a1 + (g * K2 + q) * a1s + ct * 16;
                float s0 = 0.f, s1 = 0.f;
#pragma unroll
                for (int ii = 0; ii < 16; ++ii) {
                  const float v = ct * 16 + ii < c0 ? z[ii] : 0.f;
                  const bool second = (bits[u] >> ii) & 1u;
                  acc[ii] = fmaf(v, second ? x1[u] : x0[u], acc[ii]);
                  const float vw = v * w[ii];
                  s0 += second ? 0.f : vw;
                  s1 += second ? vw : 0.f;
                }
                float* p0 = dxg + (int64_t)(2 * q) * D;
                float* p1 = dxg + (int64_t)(2 * q + 1) * D;
                *p0 = ct == 0 ? s0 : *p0 + s0;
                *p1 = ct == 0 ? s1 : *p1 + s1;
              }
            }
          }
          if (ct == 0 && (k & 1)) dxg[(int64_t)(k - 1) * D] = 0.f;  // the row the pool dropped
        }
#pragma unroll
        for (int ii = 0; ii < 16; ++ii) {
          const int ch = ct * 16 + ii;
          if (ch < c0) slab_add(dW1 + (int64_t)ch * D + d, acc[ii], first);
        }
      }
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------

static bool make_dims(int64_t B, int k, int D, int c0, int c1, int H, int dense, int C, Dims* dm,
                      size_t* lds_fwd, size_t* lds_bwd) {
  if (B < 1 || k < 10 || k > 512 || D < 1 || D > 4097 || c0 < 1 || c0 > 64 || c1 < 1 || c1 > 64 ||
      H < 1 || H > 256 || C < 1 || C > MAXC)
    return false;
  const int K2 = k / 2, P = K2 - (KT - 1);
  if (P < 1 || dense != c1 * P) return false;
  if (B * (int64_t)K2 * 4 >= ((int64_t)1 << 40)) return false;
  Dims d = {};
  d.B = B; d.k = k; d.D = D; d.c0 = c0; d.c1 = c1; d.H = H; d.C = C;
  d.K2 = K2; d.P = P; d.dense = dense; d.He = H + (H & 1); d.a1s = c0 + 1;
  d.nct = (c0 + 15) / 16;
  // graphs per pass: one until the grid holds four workgroups per CU (256 CUs), since a pass is
  // a chain of short dependent phases that only other resident workgroups hide
  int gb = (int)std::min<int64_t>(GBMAX, (B + 1023) / 1024);
  const size_t nw2 = (size_t)c1 * c0 * KT <= W2LDS ? (size_t)c1 * c0 * KT : 0;
  size_t lf = 0, lb = 0;
  for (;; --gb) {
    // forward and backward lay the same floats out first, conv2's weights after the larger
    lf = (size_t)gb * K2 * d.a1s + std::max<size_t>(STAGE, (size_t)gb * (dense + H));
    lb = (size_t)gb * K2 * d.a1s + (size_t)gb * (dense + 2 * H + C);
    if ((std::max(lf, lb) + nw2) * sizeof(float) <= kPlainLds || gb == 1) break;
  }
  d.w2off = nw2 ? (int)std::max(lf, lb) : -1;
  lf = lb = (std::max(lf, lb) + nw2) * sizeof(float);
  if (lf > kMaxLds) return false;
  d.gb = gb;
  *dm = d;
  *lds_fwd = lf;
  *lds_bwd = lb;
  return true;
}

static size_t pad64(size_t n) { return (n + 63) & ~(size_t)63; }

// slab regions of the backward workspace, in floats
struct Layout {
  int slots, sw;
  size_t dW1, db1, dW2, db2, dL1, dbL1, dL0, db0, total;
};

static Layout make_layout(const Dims& d) {
  Layout L = {};
  const int64_t npass = (d.B + d.gb - 1) / d.gb;
  const int64_t per = (int64_t)d.c0 * d.D + d.c0 + (int64_t)d.c1 * d.c0 * KT + d.c1 + d.C * d.H + d.C;
  const int64_t cap = std::max<int64_t>(8, std::min<int64_t>(kMaxSlots, kSlabBudget / per));
  L.slots = (int)std::min<int64_t>(npass, cap);
  L.sw = lgnn_s3_wgrad_partials(d.B, d.dense, d.He);
  size_t o = 0;
  const size_t S = L.slots;
  L.dW1 = o; o += pad64(S * d.c0 * d.D);
  L.db1 = o; o += pad64(S * d.c0);
  L.dW2 = o; o += pad64(S * d.c1 * d.c0 * KT);
  L.db2 = o; o += pad64(S * d.c1);
  L.dL1 = o; o += pad64(S * d.C * d.H);
  L.dbL1 = o; o += pad64(S * d.C);
  L.dL0 = o; o += pad64((size_t)L.sw * d.He * d.dense);
  L.db0 = o; o += pad64((size_t)L.sw * d.He);
  L.total = o;
  return L;
}

// lgnn_s3_wgrad addresses its operands with 32-bit byte offsets
static bool wgrad_fits(const Dims& d) {
  return (d.B + 64) * (int64_t)std::max(d.dense, d.He) * 4 < ((int64_t)1 << 31);
}

template <typename K>
static int raise_lds(K kernel, size_t lds) {
  if (lds <= kPlainLds) return LGNN_OK;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  return e == hipSuccess ? LGNN_OK : (int)e;
}

}  // namespace lgnn_drgnet_head

using namespace lgnn_drgnet_head;

extern "C" size_t lgnn_drgnet_head_workspace_bytes(int64_t num_graphs, int k, int dims, int c0,
                                                   int c1, int hidden, int classes) {
  Dims d;
  size_t lf, lb;
  const int dense = k >= 10 ? c1 * (k / 2 - (KT - 1)) : 0;
  if (!make_dims(num_graphs, k, dims, c0, c1, hidden, dense, classes, &d, &lf, &lb) ||
      !wgrad_fits(d))
    return 0;
  return make_layout(d).total * sizeof(float);
}

extern "C" int lgnn_drgnet_head_fwd(const float* x, int64_t num_graphs, int k, int dims,
                                    const float* conv1_w, const float* conv1_b, int c0,
                                    const float* conv2_w, const float* conv2_b, int c1,
                                    const float* lin0_w, const float* lin0_b, int hidden,
                                    int dense, const float* lin1_w, const float* lin1_b,
                                    int classes, const float* mask, float* logits, float* a1,
                                    uint16_t* sel, float* a2, float* h, void* stream) {
  Dims d;
  size_t lf, lb;
  if (!make_dims(num_graphs, k, dims, c0, c1, hidden, dense, classes, &d, &lf, &lb))
    return LGNN_EINVAL;
  if (!x || !conv1_w || !conv1_b || !conv2_w || !conv2_b || !lin0_w || !lin0_b || !lin1_w ||
      !lin1_b || !logits || !a1 || !sel || !a2 || !h)
    return LGNN_EINVAL;
  const int64_t npass = (d.B + d.gb - 1) / d.gb;
  const dim3 grid((unsigned)std::min<int64_t>(npass, 2048)), block(NT);
  hipStream_t s = as_stream(stream);
  if (c0 % 16 == 0) {
    if (const int e = raise_lds(&k_head_fwd<true>, lf)) return e;
    hipLaunchKernelGGL(k_head_fwd<true>, grid, block, lf, s, d, x, conv1_w, conv1_b, conv2_w,
                       conv2_b, lin0_w, lin0_b, lin1_w, lin1_b, mask, logits, a1, sel, a2, h);
  } else {
    if (const int e = raise_lds(&k_head_fwd<false>, lf)) return e;
    hipLaunchKernelGGL(k_head_fwd<false>, grid, block, lf, s, d, x, conv1_w, conv1_b, conv2_w,
                       conv2_b, lin0_w, lin0_b, lin1_w, lin1_b, mask, logits, a1, sel, a2, h);
  }
  return last_error();
}

extern "C" int lgnn_drgnet_head_bwd(const float* dlogits, const float* x, int64_t num_graphs,
                                    int k, int dims, const float* conv1_w, int c0,
                                    const float* conv2_w, int c1, const float* lin0_w, int hidden,
                                    int dense, const float* lin1_w, int classes,
                                    const float* mask, const float* a1, const uint16_t* sel,
                                    const float* a2, const float* h, float* dx, float* dh,
                                    float* dconv1_w, float* dconv1_b, float* dconv2_w,
                                    float* dconv2_b, float* dlin0_w, float* dlin0_b,
                                    float* dlin1_w, float* dlin1_b, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  Dims d;
  size_t lf, lb;
  if (!make_dims(num_graphs, k, dims, c0, c1, hidden, dense, classes, &d, &lf, &lb) ||
      !wgrad_fits(d))
    return LGNN_EINVAL;
  if (!dlogits || !x || !conv1_w || !conv2_w || !lin0_w || !lin1_w || !a1 || !sel || !a2 || !h ||
      !dx || !dh || !dconv1_w || !dconv1_b || !dconv2_w || !dconv2_b || !dlin0_w || !dlin0_b ||
      !dlin1_w || !dlin1_b || !workspace)
    return LGNN_EINVAL;
  const Layout L = make_layout(d);
  if (workspace_bytes < L.total * sizeof(float)) return LGNN_EINVAL;
  float* ws = static_cast<float*>(workspace);
  hipStream_t s = as_stream(stream);
  if (const int e = raise_lds(&k_head_bwd, lb)) return e;
  const Slabs sl = {ws + L.dW1, ws + L.db1, ws + L.dW2, ws + L.db2, ws + L.dL1, ws + L.dbL1};
  if (const int e = launch_lds(k_head_bwd, dim3((unsigned)L.slots), dim3(NT), lb, s, d, dlogits, x,
                               conv1_w, conv2_w, lin0_w, lin1_w, mask, a1, sel, a2, h, dx, dh,
                               sl)) return e;
  // dL0 [He][dense] = dh^T a2 and db0 = colsum dh: the library's weight-gradient GEMM, B in chunks
  if (const int e = lgnn_s3_wgrad(dh, d.He, a2, d.B, d.dense, 3, ws + L.dL0, L.sw, ws + L.db0,
                                  stream))
    return e;
  const float* parts[8] = {ws + L.dW1, ws + L.db1, ws + L.dW2, ws + L.db2,
                           ws + L.dL1, ws + L.dbL1, ws + L.dL0, ws + L.db0};
  const int np[8] = {L.slots, L.slots, L.slots, L.slots, L.slots, L.slots, L.sw, L.sw};
  const int64_t len[8] = {(int64_t)d.c0 * d.D, d.c0, (int64_t)d.c1 * d.c0 * KT, d.c1,
                          (int64_t)d.C * d.H, d.C, (int64_t)d.He * d.dense, d.He};
  float* outs[8] = {dconv1_w, dconv1_b, dconv2_w, dconv2_b, dlin1_w, dlin1_b, dlin0_w, dlin0_b};
  return lgnn_reduce_partials_multi(8, parts, np, len, outs, stream);
}
