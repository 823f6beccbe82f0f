// Lesion-node feature pooling for a batch, with the bilinear reinterpolation evaluated on the fly.
// Reference: src/lesion_gnn/datasets/nodes/lesions.py:147-148 (F.interpolate(features,
// size=reinterpolation, mode="bilinear"), align_corners=False) followed by :88-93
// (extract_features_by_cc: scatter mean / max over the connected components), per image. With the
// reference config (configs/config.py:15, reinterpolation=(512, 512)) the interpolated map of one
// image is 1024 x 512 x 512 fp32 = 1.07 GB, a bilinear function of a 16 x 16 x 1024 map of 1 MB:
// here that map is never stored. A pixel's value is formed from its four source taps where it is
// pooled, so a launch reads the source maps and one int16 label per pixel and channel group.
//
// k_rs_count — per image (node_ptr gives its rows of the flat outputs): label histogram (LDS per
//              workgroup, one global integer atomic per touched bin), the int16 labels (-1 for a
//              label outside the image's range, counted in *err), and, once per launch, the
//              H + W taps: source offsets and weights of every output row and column.
// k_rs_pool  — one workgroup per (image, group of CH channels). The group's source maps are staged
//              in LDS (not when the sizes are equal: the taps are the identity and the pixel is
//              read in place, bit for bit). A lane keeps one column x and walks down the rows of
//              its wave (y = wave, wave + 4, ...): its column's taps stay in registers, the row's
//              taps are wave-uniform (scalar loads), and since components are compact, a lane's
//              consecutive pixels mostly share a label: it keeps one (label, partial) run in
//              registers. Where labels change, the lanes that end a run of the same label combine
//              their partials by a butterfly over the wave (the other lanes contribute the neutral
//              element) and one of them updates the wave's private LDS bin with a plain
//              read-modify-write; labels are taken in lane order. The four waves' bins are folded
//              in wave order and divided by the count (mean). No float atomics anywhere: every
//              float operation has a fixed place in a fixed order, so two calls give the same bits.
#include <algorithm>

#include "launch.h"
#include "wg.h"

namespace lgnn_ccresample {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxSeg = LGNN_CC_POOL_MAX_SEGMENTS;  // per image, as lgnn_cc_pool
constexpr int64_t kMaxSrcBytes = LGNN_CC_POOL_RESAMPLE_MAX_SOURCE_BYTES;
constexpr size_t kPlainLds = 65536;  // dynamic LDS a launch gets without asking for more

// One output row's (or column's) two source rows (columns), as offsets into a source map, and
// their weights: torch's upsample_bilinear2d, align_corners=False.
struct Tap {
  int i0, i1;
  float w0, w1;
};

__device__ __forceinline__ Tap make_tap(int dst, int in, int out, int stride) {
  // the position in double (H + W of them per launch), so that the fp32 weight is the rounded
  // exact one: torch's fp32 scale puts up to ~18 * 2^-24 * max|f| into a pixel at odd ratios
  double src = (double)in / (double)out * ((double)dst + 0.5) - 0.5;
  src = src < 0.0 ? 0.0 : src;
  const int i0 = min((int)src, in - 1);
  const int i1 = i0 + (i0 < in - 1 ? 1 : 0);
  const float lam = (float)(src - (double)i0);
  return Tap{i0 * stride, i1 * stride, 1.f - lam, lam};
}

// the rows [base, base + n) of the flat outputs that image b owns: none if node_ptr does not
// describe rows inside [0, total); never more than the nmax the bins are sized for
struct Rows {
  int64_t base;
  int n;
};
__device__ __forceinline__ Rows image_rows(const int64_t* node_ptr, int b, int total, int nmax) {
  const int64_t r0 = node_ptr[b], r1 = node_ptr[b + 1];
  const bool ok = r0 >= 0 && r0 <= r1 && r1 <= total;
  return Rows{ok ? r0 : 0, ok ? (int)min(r1 - r0, (int64_t)nmax) : 0};
}

__global__ void __launch_bounds__(kThreads)
    k_rs_count(const int64_t* __restrict__ cc, int64_t hw, int cbi,
               const int64_t* __restrict__ node_ptr, int total, int nmax,
               int32_t* __restrict__ count, int16_t* __restrict__ lab, int32_t* __restrict__ err,
               Tap* __restrict__ taps, int h, int w, int H, int W) {
  extern __shared__ int32_t hist[];  // [nmax]
  const int b = blockIdx.x / cbi, blk = blockIdx.x - b * cbi;
  const Rows r = image_rows(node_ptr, b, total, nmax);
  for (int i = threadIdx.x; i < r.n; i += kThreads) hist[i] = 0;
  __syncthreads();
  int bad = 0;
  const int64_t per = (hw + cbi - 1) / cbi;
  const int64_t p0 = b * hw + blk * per;
  const int64_t p1 = min((b + 1) * hw, p0 + per);
  for (int64_t p = p0 + threadIdx.x; p < p1; p += kThreads) {
    const int64_t l = cc[p];
    if (l < 0 || l >= r.n) {
      ++bad;
      lab[p] = -1;
      continue;
    }
    lab[p] = (int16_t)l;
    atomicAdd(&hist[l], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < r.n; i += kThreads)
    if (hist[i]) atomicAdd(&count[r.base + i], hist[i]);
  bad = wave_sum(bad);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(err, bad);
  if (taps)  // rows first, then columns
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < (int64_t)H + W;
         i += (int64_t)gridDim.x * kThreads)
      taps[i] = i < H ? make_tap((int)i, h, H, w) : make_tap((int)(i - H), w, W, 1);
}

template <bool kMax, bool kIdent, int CH>
__global__ void __launch_bounds__(kThreads)
    k_rs_pool(const float* __restrict__ feat, int C, int h, int w,
              const int16_t* __restrict__ lab, int H, int W, const Tap* __restrict__ taps,
              const int64_t* __restrict__ node_ptr, int total, int nmax, int cgroups,
              const int32_t* __restrict__ count, float* __restrict__ out) {
  extern __shared__ float lds[];  // bins [kWaves][CH][nmax], then (not kIdent) source [CH][h * w]
  const int b = blockIdx.x / cgroups, c0 = (blockIdx.x - b * cgroups) * CH;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const Rows r = image_rows(node_ptr, b, total, nmax);
  const float init = kMax ? -__builtin_inff() : 0.f;
  auto op = [](float a, float v) { return kMax ? fmaxf(a, v) : a + v; };
  const int hw = h * w;
  const int nch = min(CH, C - c0);
  const float* f = feat + ((int64_t)b * C + c0) * hw;
  float* src = lds + kWaves * CH * nmax;
  for (int i = threadIdx.x; i < kWaves * CH * nmax; i += kThreads) lds[i] = init;
  if (!kIdent)
    for (int i = threadIdx.x; i < CH * hw; i += kThreads) src[i] = i < nch * hw ? f[i] : 0.f;
  __syncthreads();

  float* wb = lds + wave * CH * nmax;
  const int16_t* l16 = lab + (int64_t)b * H * W;
  int cur = -1;
  float acc[CH];
#pragma unroll
  for (int ch = 0; ch < CH; ++ch) acc[ch] = init;
  // The lanes of `want` end their runs. Called by the whole wave: per label among them, lowest
  // lane first, the partials meet in a butterfly (fixed order) and that lane updates the bin.
  auto flush = [&](bool want) {
    unsigned long long m = __ballot(want);
    while (m) {
      const int first = __ffsll((long long)m) - 1;
      const int L = __shfl(cur, first, 64);
      const bool mine = want && cur == L;
      const unsigned long long g = __ballot(mine);
      m &= ~g;
#pragma unroll
      for (int ch = 0; ch < CH; ++ch) {
        float s = mine ? acc[ch] : init;
        if (g & (g - 1))  // more than one lane holds this label
          for (int o = 32; o > 0; o >>= 1) s = op(s, __shfl_xor(s, o, 64));
        if (lane == first) wb[ch * nmax + L] = op(wb[ch * nmax + L], s);
      }
    }
  };
  for (int xb = 0; xb < W; xb += 64) {
    const int x = xb + lane;
    const bool in = x < W;
    Tap tx{0, 0, 0.f, 0.f};
    if (!kIdent && in) tx = taps[H + x];
    for (int y = wave; y < H; y += kWaves) {
      const int l = in ? (int)l16[(int64_t)y * W + x] : -1;
      const bool live = l >= 0;
      float v[CH];
      if (kIdent) {
#pragma unroll
        for (int ch = 0; ch < CH; ++ch)
          v[ch] = in && ch < nch ? f[(int64_t)ch * hw + (int64_t)y * W + x] : 0.f;
      } else {
        const Tap ty = taps[y];
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) {
          const float* s = src + ch * hw;
          const float top = tx.w0 * s[ty.i0 + tx.i0] + tx.w1 * s[ty.i0 + tx.i1];
          const float bot = tx.w0 * s[ty.i1 + tx.i0] + tx.w1 * s[ty.i1 + tx.i1];
          v[ch] = ty.w0 * top + ty.w1 * bot;
        }
      }
      const bool chg = live && l != cur;
      flush(chg && cur >= 0);
      if (chg) cur = l;
#pragma unroll
      for (int ch = 0; ch < CH; ++ch) acc[ch] = chg ? v[ch] : live ? op(acc[ch], v[ch]) : acc[ch];
    }
  }
  flush(cur >= 0);
  __syncthreads();

  // fold the wave bins in wave order
  for (int i = threadIdx.x; i < r.n; i += kThreads) {
    const int cnt = count[r.base + i];
    for (int ch = 0; ch < nch; ++ch) {
      float v = lds[ch * nmax + i];
      for (int wv = 1; wv < kWaves; ++wv) v = op(v, lds[(wv * CH + ch) * nmax + i]);
      if (kMax)
        v = cnt > 0 ? v : 0.f;
      else
        v = v / (float)max(cnt, 1);
      out[(r.base + i) * C + c0 + ch] = v;
    }
  }
}

static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

static bool dims_ok(int B, int H, int W) {
  return B > 0 && H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31) &&
         (int64_t)B * H * W < ((int64_t)1 << 31);
}

}  // namespace lgnn_ccresample

using namespace lgnn_ccresample;

extern "C" size_t lgnn_cc_pool_resample_workspace_bytes(int batch, int height, int width,
                                                        int total_nodes) {
  if (!dims_ok(batch, height, width) || total_nodes < 1) return 0;
  return align256((size_t)total_nodes * sizeof(int32_t)) +                  // counts
         align256((size_t)batch * height * width * sizeof(int16_t)) +       // compact labels
         align256(((size_t)height + width) * sizeof(Tap));                   // taps
}

extern "C" int lgnn_cc_pool_resample(const float* features, int batch, int channels,
                                     int src_height, int src_width, const int64_t* labels,
                                     int height, int width, const int64_t* node_ptr,
                                     int total_nodes, int max_nodes, int reduce_max, float* out,
                                     int32_t* counts_out, int32_t* err, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  if (channels <= 0 || !dims_ok(batch, height, width) || !dims_ok(1, src_height, src_width) ||
      total_nodes < 1 || max_nodes < 1 || max_nodes > kMaxSeg)
    return LGNN_EINVAL;
  const bool ident = src_height == height && src_width == width;
  const int64_t src_bytes = ident ? 0 : (int64_t)src_height * src_width * sizeof(float);
  if (src_bytes > kMaxSrcBytes) return LGNN_EINVAL;
  if (!features || !labels || !node_ptr || !out || !err || !workspace ||
      workspace_bytes < lgnn_cc_pool_resample_workspace_bytes(batch, height, width, total_nodes))
    return LGNN_EINVAL;
  hipStream_t s = as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  int32_t* count = counts_out ? counts_out : reinterpret_cast<int32_t*>(ws);
  ws += align256((size_t)total_nodes * sizeof(int32_t));
  int16_t* lab = reinterpret_cast<int16_t*>(ws);
  ws += align256((size_t)batch * height * width * sizeof(int16_t));
  Tap* taps = reinterpret_cast<Tap*>(ws);

  hipError_t e = hipMemsetAsync(count, 0, (size_t)total_nodes * sizeof(int32_t), s);
  if (e == hipSuccess) e = hipMemsetAsync(err, 0, sizeof(int32_t), s);
  if (e != hipSuccess) return (int)e;
  const int64_t hw = (int64_t)height * width;
  const int cbi = (int)std::min<int64_t>(64, std::max<int64_t>(1, hw / 4096));
  int r = launch_lds(k_rs_count, dim3((unsigned)(batch * cbi)), dim3(kThreads),
                     max_nodes * sizeof(int32_t), s, labels, hw, cbi, node_ptr, total_nodes,
                     max_nodes, count, lab, err, ident ? nullptr : taps, src_height, src_width,
                     height, width);
  if (r != LGNN_OK) return r;

  // four channels share a pixel's label, taps and run bookkeeping where their bins and source
  // maps fit the LDS a launch gets unasked; else one channel, with up to 127 KB of LDS
  const size_t per_channel = (size_t)kWaves * max_nodes * sizeof(float) + (size_t)src_bytes;
  const bool four = channels >= 4 && 4 * per_channel <= kPlainLds;
  const int ch = four ? 4 : 1, cgroups = (channels + ch - 1) / ch;
  const size_t lds = ch * per_channel;
  const dim3 grid((unsigned)((int64_t)batch * cgroups));
  one_of<false, true>(reduce_max != 0, [&](auto MAX) { one_of<false, true>(ident, [&](auto ID) {
    one_of<1, 4>(ch, [&](auto CH) {
      constexpr auto kernel = k_rs_pool<MAX, ID, CH>;
      if (lds > kPlainLds) {
        const hipError_t e =
            hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
          r = (int)e;
          return;
        }
      }
      r = launch_lds(kernel, grid, dim3(kThreads), lds, s, features, channels, src_height,
                     src_width, lab, height, width, taps, node_ptr, total_nodes, max_nodes,
                     cgroups, count, out);
    }); }); });
  return r;
}
