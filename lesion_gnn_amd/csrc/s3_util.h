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
// operand. plane_items() items in all: with b0 first the fold slot's (W_10 = W_1 W_0, its fp32
// b_10 behind its planes), one (n, k) each, then the nl layers', one (layer, n, 4 consecutive k)
// each. Run by k_wplanes (stack3.hip) or as side work of the graph build's first launch
// (graph.hip).
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
constexpr int FOLD_ITEMS = WP * WP;       // items of the fold slot
constexpr int FOLD_NT = 256;  // threads per workgroup of every kernel that runs the job
static_assert(PLANE_ITEMS % FOLD_NT == 0 && FOLD_ITEMS % FOLD_NT == 0,
              "every slot is whole workgroups: the slot test is block-uniform");
// items of the job: the fold slot's (first: its workgroups fetch the most) and the layers'
__host__ __device__ inline int plane_items(const PlaneArgs& a) {
  return (a.b0 ? FOLD_ITEMS : 0) + a.nl * PLANE_ITEMS;
}
// the fold slot's fp32 b_10 [WP], behind its planes
__host__ __device__ inline float* fold_bias(uint16_t* Wp, int nl) {
  return reinterpret_cast<float*>(Wp + (size_t)(nl + 1) * 3 * PLANE);
}

// Fold slot, item (n, k): W_10 = W_1 W_0 (in_proj folded into conv 1, exact: no activation
// between them), W_10[n][k] = sum_j W_1[n][j] W_0[j][k] in fp32 fmaf, j ascending (a fixed
// order: the same bits from every launch that runs the job), split like any other slot; every
// thread also runs b_10[n] = sum_j W_1[n][j] b_0[j] ahead of it (while its loads are in flight)
// and the k == 0 item writes it as fp32 behind the planes. Run by whole 256-thread
// workgroups, 2 rows n each (64 workgroups: the sums are the launch's longest dependent chains,
// so they are spread thin). The sums are up to 128 terms long, so no term waits for a load of
// its own: a thread fetches its column k of W_0 straight into registers (consecutive lanes,
// consecutive k: 256 B per wave and row), rows 0..63 all in flight before the first fmaf (as
// many as a wave can have outstanding) and row j + 64 into the register term j has just left,
// 64 terms ahead of its use; the workgroup's 2 rows of W_1 and b_0 (1.5 KiB of LDS, fetched
// ahead of the columns) are read as broadcasts. The build's own workgroups carry the kernel's
// registers, hence 64 and not 128 of them for the column.
// (A global load per term costs a memory round trip per term: that form held the build's first
// launch for 25 us; 8 rows per workgroup with W_0 staged through 32 KiB of LDS for 12 us.)
constexpr int FOLD_ROWS = FOLD_NT / WP;  // rows of W_10 per workgroup
struct FoldSmem {
  float w1[FOLD_ROWS][WP];
  float b0[WP];
};
__device__ __forceinline__ void wplanes_fold_item(const PlaneArgs& a, int n, int k) {
  __shared__ __attribute__((aligned(16))) FoldSmem sm;
  const int K = a.K[0], J = a.N[0], N = a.N[1];  // W_0 [J][K], W_1 [N][J]; all multiples of 4
  // (k = threadIdx.x % 128, n = the workgroup's first row + threadIdx.x / 128)
  const int t = threadIdx.x;
  // the small operands first (the barrier below waits for them alone): threads 0..63 a 16-B
  // piece of the 2 rows of W_1, threads 64..95 one of b_0; zero past the widths
  const int sr = t / (WP / 4), sp = 4 * (t % (WP / 4));
  f32x4 sv = zero4();
  if (sr < FOLD_ROWS) {
    const int sn = n - t / WP + sr;
    if (sn < N && sp < J) sv = ld4(a.W[1] + (int64_t)sn * J + sp);
  } else if (sr == FOLD_ROWS) {
    if (sp < J) sv = ld4(a.b0 + sp);
  }
  // column k of W_0 (columns past K: a valid address again, not used): a uniform row pointer
  // and one lane offset, not a lane address per row
  constexpr int RING = 64;
  const unsigned kk = k < K ? k : 0;
  const float* row = a.W[0];
  float c0[RING];
#pragma unroll
  for (int j = 0; j < RING; ++j) {
    c0[j] = row[kk];
    if (j + 1 < J) row += K;  // (rows past J: the last row again, not used)
  }
  if (sr < FOLD_ROWS) st4(&sm.w1[sr][sp], sv);
  else if (sr == FOLD_ROWS) st4(&sm.b0[sp], sv);
  __syncthreads();
  const float* w1r = sm.w1[t / WP];
  // b_10's chain first: it needs the small operands only and runs while the columns arrive
  // (in one loop with W_10's the two become packed FMAs and c0 takes twice the registers)
  float s = 0.f;
  for (int j = 0; j < J; j += 4) {
    const f32x4 c = ld4(w1r + j);
    const f32x4 bq = ld4(&sm.b0[j]);
#pragma unroll
    for (int u = 0; u < 4; ++u) s = fmaf(c[u], bq[u], s);
  }
  float v = 0.f;
#pragma unroll
  for (int j = 0; j < WP; j += 4) {
    if (j < J) {  // (uniform; no early exit: the loop unrolls, c0 stays in registers)
      const f32x4 c = ld4(w1r + j);
#pragma unroll
      for (int u = 0; u < 4; ++u) v = fmaf(c[u], c0[(j + u) % RING], v);
    }
    // rows j + 64 .. j + 67, outside the branch (a load inside one makes every wait behind the
    // join a wait for all loads); past J the last row again, not used
    if (j + RING < WP) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        c0[(j + u) % RING] = row[kk];
        if (j + u + RING + 1 < J) row += K;
      }
    }
  }
  if (k >= K) v = 0.f;  // (rows past N: W_1's row is zero)
  // four consecutive k meet in the lane of the first: one 8-byte store per plane
  f32x4 v4;
  v4[0] = v;
  v4[1] = __shfl_down(v, 1, 64);
  v4[2] = __shfl_down(v, 2, 64);
  v4[3] = __shfl_down(v, 3, 64);
  if ((k & 3) == 0) {
    u32x2 o[3];
    split4(v4, o);
    uint16_t* base = a.Wp + (size_t)a.nl * 3 * PLANE;
#pragma unroll
    for (int p = 0; p < 3; ++p)
      *reinterpret_cast<u32x2*>(base + p * PLANE + frag_index(n, perm16(k))) = o[p];
  }
  if (k == 0) fold_bias(a.Wp, a.nl)[n] = s;  // (zero past w2)
}
static_assert(LGNN_PLANE_JOB_MAX == LGNN_MAX_STACK, "plane job layers");

__device__ __forceinline__ void wplanes_item(const PlaneArgs& a, int i) {
  if (i >= plane_items(a)) return;
  if (a.b0) {
    if (i < FOLD_ITEMS) return wplanes_fold_item(a, i / WP, i % WP);
    i -= FOLD_ITEMS;
  }
  const int l = i / PLANE_ITEMS;
  const int n = (i / (WP / 4)) % WP, k = 4 * (i % (WP / 4));
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
