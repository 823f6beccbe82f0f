// Evaluation on the device (reference models/base.py:190-233 validation_step / test_step /
// logits_to_preds, the torchmetrics collections of :120-145 and the referable-DR metrics of
// metrics.py:7-83): one launch per validation batch accumulates integer counters, the loss sums
// and the referable scores into caller-held state; once per epoch every metric is computed from
// that state. State layout, definitions and the NaN cases: include/lgnn.h.
//
//   k_eval_update  one workgroup: per row argmax / round, the referable score, the loss term; the
//                  confusion matrix and referable counts in an LDS histogram added to the int64
//                  counters at the end; scores appended in row order at the device-side n_seen.
//   k_eval_rank    the pair counts behind AUROC / AUPRC: thread = sample i, the j side streamed
//                  through LDS (all lanes read one address: a broadcast, no bank conflict), integer
//                  counts added per sample with integer atomics (order-independent).
//   k_eval_final   one workgroup: sums the per-sample counts in a fixed order, then thread 0 forms
//                  every metric in double.
#include "launch.h"
#include "wg.h"

namespace {

constexpr int CT = 1024;  // k_eval_update / k_eval_final / k_eval_merge: one workgroup
constexpr int RB = 256;   // k_eval_rank: samples i per workgroup
constexpr int T = LGNN_EVAL_RANK_CHUNK;
constexpr int MAXC = LGNN_EVAL_MAX_CLASSES;

__device__ __forceinline__ float reg_term(float d, int smooth) {  // loss.hip's
  if (!smooth) return d * d;
  const float a = fabsf(d);
  return a < 1.f ? 0.5f * d * d : a - 0.5f;
}

template <bool REG>
__global__ __launch_bounds__(CT) void k_eval_update(const float* __restrict__ z,
                                                    const int64_t* __restrict__ y,
                                                    const float* __restrict__ weight, int64_t B,
                                                    int C, int smooth, int64_t* counts,
                                                    double* loss_acc, float* __restrict__ scores,
                                                    int32_t* __restrict__ positive,
                                                    int64_t capacity) {
  __shared__ int hist[MAXC * MAXC + 4];  // [target][pred], then tn fp fn tp
  __shared__ int wcount[CT / 64];
  __shared__ int nbad;
  __shared__ double red[CT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int CC = C * C;
  for (int k = tid; k < CC + 4; k += CT) hist[k] = 0;
  if (tid == 0) nbad = 0;
  const int64_t n0 = counts[CC + LGNN_EVAL_NSEEN];  // written only after the last barrier below
  __syncthreads();
  int64_t appended = 0;  // valid rows of the chunks before this one (the same in every thread)
  double num = 0.0, den = 0.0;
  for (int64_t base = 0; base < B; base += CT) {
    const int64_t i = base + tid;
    int64_t t = -1;
    if (i < B) {
      t = y[i];
      if (t < 0 || t >= C) {
        t = -1;
        atomicAdd(&nbad, 1);
      }
    }
    const bool valid = t >= 0;
    float score = 0.f;
    if (valid) {
      int pred, rpred;
      if constexpr (REG) {
        const float p = fminf(fmaxf(z[i], 0.f), (float)(C - 1));
        pred = (int)rintf(p);  // half to even, as torch.round
        rpred = pred >= 2;
        num += (double)reg_term(p - (float)t, smooth);
        den += 1.0;
      } else {
        const float* zi = z + i * C;
        float m = zi[0];
        pred = 0;
        for (int c = 1; c < C; ++c)
          if (zi[c] > m) {  // strict: the lowest index among the maxima; a NaN never wins
            m = zi[c];
            pred = c;
          }
        float mx = -INFINITY;
        for (int c = 0; c < C; ++c) mx = fmaxf(mx, zi[c]);
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += expf(zi[c] - mx);
        for (int c = 2; c < C; ++c) score += expf(zi[c] - mx) / s;
        rpred = score > 0.5f;
        const float wt = weight ? weight[t] : 1.f;
        num += (double)(wt * (mx + logf(s) - zi[t]));  // k_ce_fwd's term
        den += (double)wt;
      }
      atomicAdd(&hist[(int)t * C + pred], 1);
      atomicAdd(&hist[CC + (t >= 2 ? 2 : 0) + rpred], 1);
    }
    // this row's place among the chunk's valid rows, in row order
    const unsigned long long ballot = __ballot(valid);
    if (lane == 0) wcount[wave] = __popcll(ballot);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < CT / 64; ++w) {
      const int c = wcount[w];
      before += w < wave ? c : 0;
      total += c;
    }
    if constexpr (!REG) {
      const int64_t pos = n0 + appended + before + __popcll(ballot & ((1ull << lane) - 1ull));
      if (valid && pos < capacity) {
        scores[pos] = score;
        positive[pos] = t >= 2;
      }
    }
    appended += total;
    __syncthreads();  // wcount is rewritten by the next chunk
  }
  const double nsum = block_sum<CT>(num, red);
  const double dsum = block_sum<CT>(den, red);
  for (int k = tid; k < CC + 4; k += CT)
    if (hist[k]) counts[k] += hist[k];
  if (tid == 0) {
    counts[CC + LGNN_EVAL_NSEEN] = n0 + appended;
    counts[CC + LGNN_EVAL_NBAD] += nbad;
    loss_acc[0] += nsum;
    loss_acc[1] += dsum;
  }
}

// ws[i] = (negatives below s_i, negatives equal to s_i, positives >= s_i, negatives >= s_i) for
// every positive i; zero on entry, the j chunks of one i block are dealt over gridDim.y workgroups
__global__ __launch_bounds__(RB) void k_eval_rank(const int64_t* __restrict__ nseen,
                                                  const float* __restrict__ scores,
                                                  const int32_t* __restrict__ positive,
                                                  int64_t capacity, int* __restrict__ ws) {
  __shared__ float2 tile[T];  // (score if negative else NaN, score if positive else NaN)
  __shared__ int nneg;        // the negatives with a score (not NaN) in this workgroup's chunks
  const int64_t n = *nseen;
  if (n > capacity) return;  // overflowed: AUROC / AUPRC are NaN
  const int64_t i0 = (int64_t)blockIdx.x * RB;
  const int64_t nchunks = (n + T - 1) / T;
  if (i0 >= n || (int64_t)blockIdx.y >= nchunks) return;  // uniform over the workgroup
  const int tid = threadIdx.x;
  const int64_t i = i0 + tid;
  const bool pi = i < n && positive[i] != 0;
  const float si = i < n ? scores[i] : NAN;
  const bool wave_has = __ballot(pi) != 0ull;  // a wave of negatives has nothing to count
  if (tid == 0) nneg = 0;
  int a = 0, b = 0, c = 0;
  for (int64_t ch = blockIdx.y; ch < nchunks; ch += gridDim.y) {
    __syncthreads();
    int mine = 0;
    for (int k = tid; k < T; k += RB) {
      const int64_t j = ch * T + k;
      float sn = NAN, sp = NAN;  // past the end: compares false with everything
      if (j < n) {
        const float v = scores[j];
        if (positive[j] != 0) sp = v; else sn = v;
      }
      mine += sn == sn;
      tile[k] = make_float2(sn, sp);
    }
    if (mine) atomicAdd(&nneg, mine);
    __syncthreads();
    if (wave_has) {
#pragma unroll 8
      for (int k = 0; k < T; ++k) {
        const float2 v = tile[k];
        a += v.x < si;
        b += v.x == si;
        c += v.y >= si;
      }
    }
  }
  if (pi) {
    // the negatives at or above s_i are those not below it (none when s_i is NaN); nneg is
    // complete: every add to it precedes the loop's last barrier
    const int d = si == si ? nneg - a : 0;
    atomicAdd(ws + 4 * i + 0, a);
    atomicAdd(ws + 4 * i + 1, b);
    atomicAdd(ws + 4 * i + 2, c);
    atomicAdd(ws + 4 * i + 3, d);
  }
}

__device__ __forceinline__ double ratio0(double a, double b) { return b != 0.0 ? a / b : 0.0; }

__global__ __launch_bounds__(CT) void k_eval_final(const int64_t* __restrict__ counts,
                                                   const double* __restrict__ loss_acc,
                                                   int64_t capacity, int C, int regression,
                                                   const int* __restrict__ ws,
                                                   double* __restrict__ result) {
  __shared__ double red[CT / 64];
  __shared__ long long ired[CT / 64];
  __shared__ long long rowsum[MAXC], colsum[MAXC];
  __shared__ long long cnt[MAXC * MAXC + LGNN_EVAL_EXTRA];  // the counters: thread 0's serial part
  __shared__ double lacc[2];                                // reads no global memory
  const int tid = threadIdx.x;
  const int CC = C * C;
  for (int k = tid; k < CC + LGNN_EVAL_EXTRA; k += CT) cnt[k] = counts[k];
  if (tid < 2) lacc[tid] = loss_acc[tid];
  const int64_t n = counts[CC + LGNN_EVAL_NSEEN];
  const bool ranked = !regression && n <= capacity;
  long long twice = 0;  // sum_i 2 gt_i + eq_i
  double ap = 0.0;      // sum_i tp_i / (tp_i + fp_i)
  if (ranked) {
    // ws is zero wherever k_eval_rank added nothing (the negatives, and a positive whose score
    // is NaN): such a sample adds 0 to both sums. 16-B loads, independent of one another.
    const int4* __restrict__ ws4 = reinterpret_cast<const int4*>(ws);
#pragma unroll 4
    for (int64_t i = tid; i < n; i += CT) {
      const int4 v = ws4[i];
      twice += 2ll * v.x + v.y;
      const int at_or_above = v.z + v.w;
      ap += at_or_above > 0 ? (double)v.z / (double)at_or_above : 0.0;
    }
  }
  const long long twice_sum = block_sum<CT>(twice, ired);
  const double ap_sum = block_sum<CT>(ap, red);
  if (tid < C) {
    long long r = 0;
    for (int j = 0; j < C; ++j) r += cnt[tid * C + j];
    rowsum[tid] = r;
  } else if (tid >= MAXC && tid < MAXC + C) {
    const int j = tid - MAXC;
    long long s = 0;
    for (int i = 0; i < C; ++i) s += cnt[i * C + j];
    colsum[j] = s;
  }
  __syncthreads();
  if (tid != 0) return;
  const double dn = (double)n;
  long long trace = 0, wo = 0;
  double we = 0.0;  // sum_ij (i - j)^2 rows_i cols_j: n times the expected weighted disagreement
  for (int i = 0; i < C; ++i)
    for (int j = 0; j < C; ++j) {
      const long long w = (long long)(i - j) * (i - j);
      wo += w * cnt[i * C + j];
      we += (double)w * (double)rowsum[i] * (double)colsum[j];
    }
  double f1 = 0.0, prec = 0.0, rec = 0.0;
  int present = 0;
  for (int k = 0; k < C; ++k) {
    const long long tp = cnt[k * C + k], fp = colsum[k] - tp, fn = rowsum[k] - tp;
    trace += tp;
    if (tp + fp + fn == 0) continue;  // in neither the predictions nor the targets: left out
    ++present;
    f1 += ratio0((double)(2 * tp), (double)(2 * tp + fp + fn));
    prec += ratio0((double)tp, (double)(tp + fp));
    rec += ratio0((double)tp, (double)(tp + fn));
  }
  const long long tn = cnt[CC + LGNN_EVAL_TN], rfp = cnt[CC + LGNN_EVAL_FP];
  const long long rfn = cnt[CC + LGNN_EVAL_FN], rtp = cnt[CC + LGNN_EVAL_TP];
  const long long npos = rfn + rtp, nneg = tn + rfp;
  result[LGNN_EVAL_R_MICRO_ACC] = ratio0((double)trace, dn);
  result[LGNN_EVAL_R_KAPPA] = 1.0 - dn * (double)wo / we;  // 0 / 0: NaN
  result[LGNN_EVAL_R_MACRO_F1] = ratio0(f1, (double)present);
  result[LGNN_EVAL_R_MACRO_PRECISION] = ratio0(prec, (double)present);
  result[LGNN_EVAL_R_MACRO_RECALL] = ratio0(rec, (double)present);
  result[LGNN_EVAL_R_ACC] = ratio0((double)(rtp + tn), dn);
  result[LGNN_EVAL_R_F1] = ratio0((double)(2 * rtp), (double)(2 * rtp + rfp + rfn));
  result[LGNN_EVAL_R_PRECISION] = ratio0((double)rtp, (double)(rtp + rfp));
  result[LGNN_EVAL_R_RECALL] = ratio0((double)rtp, (double)(rtp + rfn));
  result[LGNN_EVAL_R_AUROC] = ranked && npos > 0 && nneg > 0
                                  ? (double)twice_sum / (2.0 * (double)npos * (double)nneg)
                                  : (double)NAN;
  result[LGNN_EVAL_R_AUPRC] = ranked && npos > 0 ? ap_sum / (double)npos : (double)NAN;
  result[LGNN_EVAL_R_LOSS] = ratio0(lacc[0], lacc[1]);
  result[LGNN_EVAL_R_NSEEN] = dn;
  result[LGNN_EVAL_R_NBAD] = (double)cnt[CC + LGNN_EVAL_NBAD];
  result[LGNN_EVAL_R_OVERFLOW] = !regression && n > capacity ? 1.0 : 0.0;
  result[LGNN_EVAL_RESULTS - 1] = 0.0;
}

__global__ __launch_bounds__(CT) void k_eval_merge(int C, int64_t* counts, double* loss_acc,
                                                   float* __restrict__ scores,
                                                   int32_t* __restrict__ positive,
                                                   const int64_t* __restrict__ src_counts,
                                                   const double* __restrict__ src_loss_acc,
                                                   const float* __restrict__ src_scores,
                                                   const int32_t* __restrict__ src_positive,
                                                   int64_t capacity) {
  const int tid = threadIdx.x;
  const int CC = C * C;
  const int64_t nd = counts[CC + LGNN_EVAL_NSEEN], ns = src_counts[CC + LGNN_EVAL_NSEEN];
  __syncthreads();  // every thread holds dst's n_seen before it is added to
  if (scores) {
    const int64_t stored = ns < capacity ? ns : capacity;
    for (int64_t k = tid; k < stored; k += CT) {
      const int64_t pos = nd + k;
      if (pos < capacity) {
        scores[pos] = src_scores[k];
        positive[pos] = src_positive[k];
      }
    }
  }
  for (int k = tid; k < CC + LGNN_EVAL_EXTRA; k += CT) counts[k] += src_counts[k];
  if (tid == 0) {
    loss_acc[0] += src_loss_acc[0];
    loss_acc[1] += src_loss_acc[1];
  }
}

}  // namespace

extern "C" int lgnn_eval_update(const float* z, const int64_t* target, const float* weight,
                                int64_t B, int C, int regression, int smooth_l1, int64_t* counts,
                                double* loss_acc, float* scores, int32_t* positive,
                                int64_t capacity, void* stream) {
  if (B <= 0 || B >= (1ll << 31) || C < 1 || C > MAXC || !z || !target || !counts || !loss_acc)
    return LGNN_EINVAL;
  if (regression) {
    hipLaunchKernelGGL(k_eval_update<true>, dim3(1), dim3(CT), 0, as_stream(stream), z, target,
                       nullptr, B, C, smooth_l1, counts, loss_acc, nullptr, nullptr, 0);
  } else {
    if (!scores || !positive || capacity < 0 || capacity >= (1ll << 31)) return LGNN_EINVAL;
    hipLaunchKernelGGL(k_eval_update<false>, dim3(1), dim3(CT), 0, as_stream(stream), z, target,
                       weight, B, C, 0, counts, loss_acc, scores, positive, capacity);
  }
  return last_error();
}

extern "C" size_t lgnn_eval_workspace_bytes(int64_t capacity) {
  return capacity > 0 ? (size_t)capacity * 4 * sizeof(int) : 0;
}

extern "C" int lgnn_eval_compute(const int64_t* counts, const double* loss_acc,
                                 const float* scores, const int32_t* positive, int64_t capacity,
                                 int C, int regression, double* result, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  if (C < 1 || C > MAXC || !counts || !loss_acc || !result) return LGNN_EINVAL;
  int* ws = static_cast<int*>(workspace);
  if (regression) {
    capacity = 0;
  } else {
    if (!scores || !positive || capacity < 0 || capacity >= (1ll << 31)) return LGNN_EINVAL;
    if (capacity > 0 && (!ws || workspace_bytes < lgnn_eval_workspace_bytes(capacity)))
      return LGNN_ENOSPC;
    if (reinterpret_cast<uintptr_t>(ws) & 15) return LGNN_EINVAL;  // read with 16-B loads
  }
  if (capacity > 0) {
    hipError_t e = hipMemsetAsync(ws, 0, lgnn_eval_workspace_bytes(capacity), as_stream(stream));
    if (e != hipSuccess) return (int)e;
    const dim3 grid((unsigned)((capacity + RB - 1) / RB), LGNN_EVAL_RANK_SPLIT);
    if (const int e = launch(k_eval_rank, grid, dim3(RB), as_stream(stream),
                             counts + C * C + LGNN_EVAL_NSEEN, scores, positive, capacity,
                             ws)) return e;
  }
  return launch(k_eval_final, dim3(1), dim3(CT), as_stream(stream), counts, loss_acc, capacity, C,
                regression, ws, result);
}

extern "C" int lgnn_eval_merge(int C, int64_t* counts, double* loss_acc, float* scores,
                               int32_t* positive, const int64_t* src_counts,
                               const double* src_loss_acc, const float* src_scores,
                               const int32_t* src_positive, int64_t capacity, void* stream) {
  if (C < 1 || C > MAXC || !counts || !loss_acc || !src_counts || !src_loss_acc ||
      counts == src_counts)
    return LGNN_EINVAL;
  const bool stored = scores || positive || src_scores || src_positive;
  if (stored && (!scores || !positive || !src_scores || !src_positive || capacity < 0))
    return LGNN_EINVAL;
  return launch(k_eval_merge, dim3(1), dim3(CT), as_stream(stream), C, counts, loss_acc, scores,
                positive, src_counts, src_loss_acc, src_scores, src_positive, capacity);
}
