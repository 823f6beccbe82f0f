// Split-3 helpers shared by the fused GCN stack kernels (stack3.hip forward, stack3_bwd.hip
// backward): bf16 plane splitting, the six-product MFMA, the perm16 feature order, LDS image
// addressing, weight-plane fragment order.
#pragma once
#include "common.h"
#include "tile_util.h"

namespace lgnn_s3 {
using namespace lgnn_tile;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int WP = 128;           // padded width of the weight planes and the H image
constexpr int PLANE = WP * WP;    // bf16 elements per weight plane
constexpr int AROW = WP * 2;      // bytes per H-image row (chunk-swizzled, no padding)
constexpr int ADJ_LD = 72;        // Â plane row stride in bf16 (144 B: conflict-free b128 rows)
constexpr int ADJ_PLANE = TM * ADJ_LD * 2;  // bytes per Â plane
// one tile's fp32 Â [target][source] as the split-3 forward hands it to the fused backward (the
// forward's LDS sum, row-major: 16 chunks of 1 KiB, one direct-to-LDS wave load each)
constexpr int ADJT_TILE_BYTES = TM * TM * 4;
static_assert(ADJT_TILE_BYTES == LGNN_S3_ADJT_TILE_BYTES && ADJT_TILE_BYTES % 1024 == 0, "");

__device__ __forceinline__ constexpr int perm16(int k) {
  return (k & ~12) | ((k & 4) << 1) | ((k & 8) >> 1);
}

// (a, b) -> three packed bf16 pairs (a in the low half), x = hi + mid + lo to 2^-24.
struct Split2 {
  uint32_t p[3];
};
__device__ __forceinline__ Split2 split2(float a, float b) {
  Split2 s;
  f32x2 v = {a, b};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const uint32_t q = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
    s.p[i] = q;
    if (i < 2) {
      const f32x2 back = {__uint_as_float(q << 16), __uint_as_float(q & 0xffff0000u)};
      v -= back;
    }
  }
  return s;
}

// four consecutive fp32 -> three planes of four bf16 (8 bytes each)
__device__ __forceinline__ void split4(f32x4 v, u32x2 (&o)[3]) {
  const Split2 a = split2(v[0], v[1]), b = split2(v[2], v[3]);
#pragma unroll
  for (int p = 0; p < 3; ++p) o[p] = u32x2{a.p[p], b.p[p]};
}

__device__ __forceinline__ f32x16 mfma16(u32x4 a, u32x4 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a),
                                                 __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// c += a.b at fp32 accuracy: the six plane products, smallest first.
__device__ __forceinline__ f32x16 mfma_s3(const u32x4 (&a)[3], const u32x4 (&b)[3], f32x16 c) {
  c = mfma16(a[2], b[0], c);
  c = mfma16(a[1], b[1], c);
  c = mfma16(a[0], b[2], c);
  c = mfma16(a[1], b[0], c);
  c = mfma16(a[0], b[1], c);
  return mfma16(a[0], b[0], c);
}
// b exact in bf16 (b_mid = b_lo = 0): three products.
__device__ __forceinline__ f32x16 mfma_s3_bexact(const u32x4 (&a)[3], u32x4 b0, f32x16 c) {
  c = mfma16(a[2], b0, c);
  c = mfma16(a[1], b0, c);
  return mfma16(a[0], b0, c);
}

// a exact in bf16 (a_mid = a_lo = 0): three products.
__device__ __forceinline__ f32x16 mfma_s3_aexact(u32x4 a0, const u32x4 (&b)[3], f32x16 c) {
  c = mfma16(a0, b[2], c);
  c = mfma16(a0, b[1], c);
  return mfma16(a0, b[0], c);
}

// Byte offset of (row, 4-aligned feature k) in an H-image plane: position perm16(k), 16-B chunk
// XOR-swizzled by row & 15 so a b128 read of one chunk by 16 rows is conflict-free.
__device__ __forceinline__ int ap_off(int row, int k) {
  const int p = perm16(k);
  return row * AROW + ((((p >> 3) ^ (row & 15))) << 4) + ((p & 7) << 1);
}
__device__ __forceinline__ int ap_chunk(int row, int c) {
  return row * AROW + ((c ^ (row & 15)) << 4);
}

__device__ __forceinline__ u32x4 lds16(const unsigned char* p) {
  return *reinterpret_cast<const u32x4*>(p);
}

// The bf16 A image of the linear kernels (bflin.hip, s3gemm.hip): BK k per chunk, 128-B rows,
// 16-B chunk XOR-swizzled by (row >> 1) & 7: the 16 rows of a ds_read_b128 lane group
// ({0-3, 12-15, 20-27} / {4-11, 16-19, 28-31}, MI355X_MICROARCH.md §LDS) land in 16 distinct 16-B
// bank slots (an (row & 7) key pairs rows 8 apart on one slot: 2-way conflicts, measured 40 %
// extra LDS cycles)
constexpr int BK = 64;           // k per chunk
constexpr int ROWB = BK * 2;     // bytes per image row (bf16)
constexpr int OOB = 0x7ff00000;  // buffer offset past every range: the load returns 0
__device__ __forceinline__ int swz(int row, int chunk) {
  return row * ROWB + ((chunk ^ ((row >> 1) & 7)) << 4);
}
// a value through an empty asm: a select feeding a buffer offset stays a v_cndmask instead of being
// sunk into two branch-guarded loads (whose join makes the wait-count pass drain to vmcnt(0))
__device__ __forceinline__ int opaque(int x) {
  asm volatile("" : "+v"(x));
  return x;
}
__device__ __forceinline__ uint32_t ldb32(Buf b, int off) {
  return __builtin_amdgcn_raw_buffer_load_b32(b, off, 0, 0);
}
__device__ __forceinline__ void sts8(unsigned char* p, u32x2 v) {
  *reinterpret_cast<u32x2*>(p) = v;
}

// element index of (row, phys position) within one fragment-ordered 128 x 128 plane
__device__ __forceinline__ int frag_index(int row, int phys) {
  return ((((row >> 5) * 8 + (phys >> 4)) * 2 + ((phys >> 3) & 1)) * 32 + (row & 31)) * 8 +
         (phys & 7);
}

// Weight planes: W_l [N][K] fp32 -> bf16 planes of W_l[n][perm16(k)], zero-padded to 128 x 128,
// stored in MFMA fragment order so that one wave's load of a k-step fragment is 1 KiB contiguous:
//   Wp[l][plane][n / 32][s][h][n % 32][8]  holds  phys positions 16 s + 8 h .. + 7 of row n
// (lane h * 32 + n % 32 of wave n / 32 loads k-step s with one 16-B load). With WpT also the
// transposed planes (rows k, positions perm16(n)) in the same order: the backward's dH = G W_l
// operand. Item i = one (slot, n, 4 consecutive k), plane_items() in all: the nl layers' and, with
// b0, the fold slot's (W_10 = W_1 W_0, its fp32 b_10 behind it). Run by
// k_wplanes (stack3.hip) or as side work of the graph build's first launch (graph.hip).
struct PlaneArgs {
  const float* W[LGNN_MAX_STACK];
  int N[LGNN_MAX_STACK];
  int K[LGNN_MAX_STACK];
  int nl;
  uint16_t* Wp;
  uint16_t* WpT;  // nullable
  const float* b0;  // fold slot (LGNN_PLANE_JOB_FOLD): in_proj's bias; nullptr = no fold slot
};
constexpr int PLANE_ITEMS = WP * WP / 4;  // items per layer
// items of the job: the layers' and, with the fold, the fold slot's
__host__ __device__ inline int plane_items(const PlaneArgs& a) {
  return (a.nl + (a.b0 ? 1 : 0)) * PLANE_ITEMS;
}
// the fold slot's fp32 b_10 [WP], behind its planes
__host__ __device__ inline float* fold_bias(uint16_t* Wp, int nl) {
  return reinterpret_cast<float*>(Wp + (size_t)(nl + 1) * 3 * PLANE);
}

// Fold slot, item (n, 4 consecutive k): W_10 = W_1 W_0 (in_proj folded into conv 1, exact: no
// activation between them), W_10[n][k..k+3] = sum_j W_1[n][j] W_0[j][k..k+3] in fp32 fmaf, j
// ascending (a fixed order: the same bits from every launch that runs the job), split like any
// other slot; the k == 0 items also write b_10[n] = sum_j W_1[n][j] b_0[j] as fp32 behind it.
// Run by whole 256-thread workgroups (a slot's items start at a multiple of 256: the slot test
// is block-uniform), 8 rows n each. The sums are 128 terms long, so nothing is loaded inside
// them: the workgroup's 8 rows of W_1, b_0 and W_0 (two halves of 64 rows, 36.5 KiB of LDS in
// all) are fetched by loads that are all in flight at once, each element once per workgroup, and
// the fmaf chains read LDS. (A global load per term costs a memory round trip per term and
// every W_0 element is wanted by 128 rows: that form held the build's first launch for 25 us.)
constexpr int FOLD_NT = 256;   // threads per workgroup of every kernel that runs the job
constexpr int FOLD_HALF = 64;  // rows of W_0 staged at a time
struct FoldSmem {
  float w0[FOLD_HALF][WP];
  float w1[FOLD_NT / (WP / 4)][WP];
  float b0[WP];
};
__device__ __forceinline__ void wplanes_fold_item(const PlaneArgs& a, int n, int k) {
  __shared__ __attribute__((aligned(16))) FoldSmem sm;
  const int K = a.K[0], J = a.N[0], N = a.N[1];  // W_0 [J][K], W_1 [N][J]; all multiples of 4
  // (k = 4 (threadIdx.x % 32), n = the workgroup's first row + threadIdx.x / 32)
  const int t = threadIdx.x, tr = t / (WP / 4);
  constexpr int PER = FOLD_HALF * WP / 4 / FOLD_NT;  // float4 of a half per thread
  // every load up front; what lies past a width is zero, so the padding needs no branch below
  f32x4 g[2][PER];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int j = FOLD_HALF * h + tr + (FOLD_NT / (WP / 4)) * u;
      g[h][u] = (j < J && k < K) ? ld4(a.W[0] + (int64_t)j * K + k) : zero4();
    }
  st4(&sm.w1[tr][k], (n < N && k < J) ? ld4(a.W[1] + (int64_t)n * J + k) : zero4());
  if (t < WP / 4) st4(&sm.b0[k], k < J ? ld4(a.b0 + k) : zero4());
  f32x4 v = zero4();
  float s = 0.f;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (h) __syncthreads();  // the first half is read
#pragma unroll
    for (int u = 0; u < PER; ++u) st4(&sm.w0[tr + (FOLD_NT / (WP / 4)) * u][k], g[h][u]);
    __syncthreads();
    const int je = J - FOLD_HALF * h < FOLD_HALF ? J - FOLD_HALF * h : FOLD_HALF;
    for (int j = 0; j < je; j += 4) {
      const f32x4 c = ld4(&sm.w1[tr][FOLD_HALF * h + j]);
      const f32x4 bq = ld4(&sm.b0[FOLD_HALF * h + j]);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const f32x4 r = ld4(&sm.w0[j + u][k]);
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = fmaf(c[u], r[q], v[q]);
        s = fmaf(c[u], bq[u], s);
      }
    }
  }
  u32x2 o[3];
  split4(v, o);
  uint16_t* base = a.Wp + (size_t)a.nl * 3 * PLANE;
#pragma unroll
  for (int p = 0; p < 3; ++p)
    *reinterpret_cast<u32x2*>(base + p * PLANE + frag_index(n, perm16(k))) = o[p];
  if (k == 0) fold_bias(a.Wp, a.nl)[n] = s;  // (zero past w2)
}
static_assert(LGNN_PLANE_JOB_MAX == LGNN_MAX_STACK, "plane job layers");

__device__ __forceinline__ void wplanes_item(const PlaneArgs& a, int i) {
  if (i >= plane_items(a)) return;
  const int l = i / PLANE_ITEMS;
  const int n = (i / (WP / 4)) % WP, k = 4 * (i % (WP / 4));
  if (l >= a.nl) return wplanes_fold_item(a, n, k);
  const int N = a.N[l], K = a.K[l];
  const f32x4 v = (n < N && k < K) ? ld4(a.W[l] + (int64_t)n * K + k) : zero4();
  u32x2 o[3];
  split4(v, o);
  uint16_t* base = a.Wp + (size_t)l * 3 * PLANE;
#pragma unroll
  for (int p = 0; p < 3; ++p)
    *reinterpret_cast<u32x2*>(base + p * PLANE + frag_index(n, perm16(k))) = o[p];
  if (a.WpT) {
    uint16_t* bt = a.WpT + (size_t)l * 3 * PLANE;
    const int pn = perm16(n);
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      bt[p * PLANE + frag_index(k + 0, pn)] = (uint16_t)(o[p][0] & 0xffffu);
      bt[p * PLANE + frag_index(k + 1, pn)] = (uint16_t)(o[p][0] >> 16);
      bt[p * PLANE + frag_index(k + 2, pn)] = (uint16_t)(o[p][1] & 0xffffu);
      bt[p * PLANE + frag_index(k + 3, pn)] = (uint16_t)(o[p][1] >> 16);
    }
  }
}

// host: the plane job of lgnn_weight_planes' arguments (LGNN_EINVAL on a bad shape)
// nl may carry LGNN_PLANE_JOB_FOLD: W[layers] is then b_0 and the fold slot is written too
inline int plane_args(int nl, const float* const* W, const int* widths, uint16_t* planes,
                      uint16_t* planes_t, PlaneArgs& a) {
  const bool fold = nl > 0 && (nl & LGNN_PLANE_JOB_FOLD);
  if (fold) nl &= ~LGNN_PLANE_JOB_FOLD;
  if (nl < 1 || nl > LGNN_MAX_STACK || !W || !widths || !planes) return LGNN_EINVAL;
  if (fold && (nl < 2 || nl > LGNN_PLANE_JOB_MAX - 1 || !W[nl])) return LGNN_EINVAL;
  a = PlaneArgs{};
  a.b0 = fold ? W[nl] : nullptr;
  for (int l = 0; l < nl; ++l) {
    const int K = widths[l], N = widths[l + 1];
    if (!W[l] || K < 4 || N < 4 || K > WP || N > WP || K % 4 || N % 4) return LGNN_EINVAL;
    a.W[l] = W[l];
    a.N[l] = N;
    a.K[l] = K;
  }
  a.nl = nl;
  a.Wp = planes;
  a.WpT = planes_t;
  return LGNN_OK;
}

// threadIdx.x through an empty asm: addresses derived from it cannot be hoisted out of the tile
// loop or merged across phases (held over the whole loop they cost ~60 registers); each phase
// recomputes its own in a few VALU ops.
__device__ __forceinline__ int fresh_tid() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

// ELU(alpha = 1) as exp2-based exp(min(x, 0)) - 1: five VALU ops. Against PyTorch's expm1 form
// the absolute difference is below 1e-7 (v_exp_f32 is ~1 ulp; the argument's rounding moves
// exp(x) by at most |x| e^x 2^-24 ln 2 <= 2.3e-8), i.e. fp32 rounding level for |ELU| <= 1.
__device__ __forceinline__ float elu_s3(float x) {
  const float e = __builtin_amdgcn_exp2f(fminf(x, 0.f) * 1.44269504088896341f) - 1.f;
  return x > 0.f ? x : e;
}

}  // namespace lgnn_s3
