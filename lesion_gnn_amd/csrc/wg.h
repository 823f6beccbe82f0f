// Workgroup scan and sum primitives (wave64), and the one-workgroup exclusive scan kernel that
// turns counts into offsets. Every "counts -> offsets" site of the library is built from these.
#pragma once
#include "common.h"

// Inclusive scan over the 64 lanes of a wave. Integer T (int32_t, int64_t).
template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

// One tile of a workgroup exclusive scan over NT threads: thread t passes its value of this tile
// and gets carry + the sum of the values of the threads below it; the uniform carry is advanced
// by the tile's total. s_wave: NT / 64 words of LDS. Two barriers, the second after the last read
// of s_wave, so the next tile may follow at once. The caller owns the loads and the stores
// (thread t of a tile owns element tile + t: coalesced, and no thread reads what another wrote).
template <int NT, typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T& carry, T* s_wave) {
  const int wave = threadIdx.x >> 6;
  const T incl = wave_inclusive_scan(v);
  if ((threadIdx.x & 63) == 63) s_wave[wave] = incl;
  __syncthreads();
  T before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const T s = s_wave[w];
    before += w < wave ? s : 0;
    all += s;
  }
  const T at = carry + before + incl - v;
  carry += all;
  __syncthreads();  // s_wave is rewritten by the next tile
  return at;
}

// Sum over the 64 lanes of a wave (every lane gets it), by the xor tree 32, 16, ... 1.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Sum over a workgroup of NT threads (every thread gets it), in a fixed order: the lanes of each
// wave by wave_sum's xor tree, then the wave totals added to 0 in ascending wave order. The order
// is a contract: the float and double callers (loss.hip, metrics.hip) are bitwise reproducible
// because of it. red: NT / 64 words of LDS.
template <int NT, typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
  v = wave_sum(v);
  __syncthreads();  // red may still be read from a previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  T t = 0;
  for (int w = 0; w < NT / 64; ++w) t += red[w];
  return t;
}

// out[i] = sum of in[0..i) for i in [0, n], so out[n] is the total (written for n == 0 too). One
// workgroup of kScanTile threads, tiles of kScanTile elements, the carry in order.
constexpr int kScanTile = 1024;

template <typename In, typename Out>
__global__ __launch_bounds__(kScanTile) void k_exclusive_scan(const In* __restrict__ in, int64_t n,
                                                              Out* __restrict__ out) {
  __shared__ Out s_wave[kScanTile / 64];
  Out carry = 0;
  for (int64_t tile = 0; tile < n; tile += kScanTile) {
    const int64_t i = tile + threadIdx.x;
    const Out at = block_exclusive_scan<kScanTile>(i < n ? (Out)in[i] : (Out)0, carry, s_wave);
    if (i < n) out[i] = at;
  }
  if (threadIdx.x == 0) out[n] = carry;
}

template <typename In, typename Out>
inline void launch_exclusive_scan(const In* in, int64_t n, Out* out, hipStream_t stream) {
  hipLaunchKernelGGL((k_exclusive_scan<In, Out>), dim3(1), dim3(kScanTile), 0, stream, in, n, out);
}
