// Fundus image preprocessing (include/lgnn.h, "Fundus image preprocessing"): the bounding box of
// the pixels with red above a threshold, then crop -> resize (8-bit INTER_LINEAR in integers, the
// mask INTER_NEAREST) -> centre pad -> normalise -> [3, S, S], for a batch of uint8 RGB images of
// different sizes. The host pointer and size tables travel as by-value kernel arguments,
// LGNN_FUNDUS_MAX_IMAGES images per launch.
#include <cmath>

#include "launch.h"

namespace {

struct FundusImages {
  const uint8_t* img[LGNN_FUNDUS_MAX_IMAGES];   // [H][W][3]
  const uint8_t* mask[LGNN_FUNDUS_MAX_IMAGES];  // [H][W], or all NULL
  int H[LGNN_FUNDUS_MAX_IMAGES];
  int W[LGNN_FUNDUS_MAX_IMAGES];
};

// ---------------------------------------------------------------------------------------------
// the box pass: every byte of every image is read once
// ---------------------------------------------------------------------------------------------

constexpr int kBoxThreads = 256;
constexpr int kBoxMinShare = 1024;   // 16-pixel groups a workgroup takes before another one helps
constexpr int kBoxMaxWorkgroups = 256;  // per image

// The workgroups of an H x W image and the 16-pixel groups each takes (its share): workgroup b
// owns groups [b * share, (b + 1) * share), counted from the image's first 16-byte-aligned byte.
__host__ __device__ inline int box_share(int H, int W, int* workgroups) {
  const int groups = (H * W + 15) / 16;  // H, W <= 16384: fits
  int n = (groups + kBoxMinShare - 1) / kBoxMinShare;
  n = n < 1 ? 1 : n > kBoxMaxWorkgroups ? kBoxMaxWorkgroups : n;
  const int share = (groups + n - 1) / n;
  *workgroups = (groups + share - 1) / share;
  return share;
}

// Which of the 16 red bytes of 48 consecutive bytes are >= ti; the first red byte is byte R.
template <int R>
__device__ __forceinline__ unsigned lit16(const uint32_t (&d)[12], unsigned ti) {
  unsigned m = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int k = R + 3 * j;
    const unsigned v = (d[k >> 2] >> ((k & 3) * 8)) & 255u;
    m |= (v >= ti ? 1u : 0u) << j;
  }
  return m;
}

struct Box {
  int x0, x1, y0, y1;  // min and max of x and of y over the lit pixels seen
  __device__ __forceinline__ void add(int x, int y) {
    x0 = min(x0, x), x1 = max(x1, x), y0 = min(y0, y), y1 = max(y1, y);
  }
};

// acc [images][4], zeroed: max over the lit pixels of (W - x, x + 1, H - y, y + 1), so that 0
// means "no lit pixel" and the four words combine with atomicMax alone. Lit: red >= ti.
//
// An image is H * W * 3 bytes at any alignment. From its first 16-byte-aligned byte on, every 48
// bytes (three 16-byte loads of one lane) hold exactly 16 pixels' red bytes, the first of them
// at byte R = (3 - head % 3) % 3 of the group (head: the bytes in front of the aligned one). The
// pixels whose red byte lies in front of the first group or behind the last one (fewer than 6 +
// 16) are read byte by byte by the image's first workgroup. Nothing outside the image is read.
__global__ __launch_bounds__(kBoxThreads) void k_fundus_box(FundusImages im, unsigned ti,
                                                           int32_t* __restrict__ acc) {
  const int b = blockIdx.y;
  const int H = im.H[b], W = im.W[b];
  int workgroups;
  const int share = box_share(H, W, &workgroups);
  if ((int)blockIdx.x >= workgroups) return;
  const uint8_t* __restrict__ base = im.img[b];
  const int64_t bytes = (int64_t)H * W * 3;
  const int64_t align = (16 - (int)(reinterpret_cast<uintptr_t>(base) & 15)) & 15;
  const int head = (int)(align < bytes ? align : bytes);
  const int groups = (int)((bytes - head) / 48);
  const int R = (3 - head % 3) % 3;
  const int first = (head + R) / 3;  // the first group's first pixel
  const int lo = (int)blockIdx.x * share, hi = min(lo + share, groups);
  Box box = {INT_MAX, -1, INT_MAX, -1};
  for (int g = lo + (int)threadIdx.x; g < hi; g += kBoxThreads) {
    const uint4* q = reinterpret_cast<const uint4*>(base + head + (int64_t)48 * g);
    const uint4 q0 = q[0], q1 = q[1], q2 = q[2];
    const uint32_t d[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
    const unsigned m = R == 0 ? lit16<0>(d, ti) : R == 1 ? lit16<1>(d, ti) : lit16<2>(d, ti);
    if (m == 0) continue;
    const unsigned p = (unsigned)(first + 16 * g);
    const int y = (int)(p / (unsigned)W), x = (int)(p - (unsigned)y * (unsigned)W);
    if (x + 16 <= W) {  // the 16 pixels are in one row
      box.add(x + __builtin_ctz(m), y);
      box.add(x + 31 - __builtin_clz(m), y);
    } else {
      for (unsigned rest = m; rest; rest &= rest - 1) {
        const int xx = x + __builtin_ctz(rest);
        box.add(xx % W, y + xx / W);
      }
    }
  }
  if (blockIdx.x == 0) {  // the pixels in front of the first group and behind the last
    const int after = first + 16 * groups, n = first + (H * W - after);
    for (int t = threadIdx.x; t < n; t += kBoxThreads) {
      const int p = t < first ? t : after + (t - first);
      if (base[(int64_t)3 * p] >= ti) box.add(p % W, p / W);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    box.x0 = min(box.x0, __shfl_xor(box.x0, o, 64));
    box.x1 = max(box.x1, __shfl_xor(box.x1, o, 64));
    box.y0 = min(box.y0, __shfl_xor(box.y0, o, 64));
    box.y1 = max(box.y1, __shfl_xor(box.y1, o, 64));
  }
  __shared__ Box s_box[kBoxThreads / 64];
  if ((threadIdx.x & 63) == 0) s_box[threadIdx.x >> 6] = box;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kBoxThreads / 64; ++w) {
      box.x0 = min(box.x0, s_box[w].x0), box.x1 = max(box.x1, s_box[w].x1);
      box.y0 = min(box.y0, s_box[w].y0), box.y1 = max(box.y1, s_box[w].y1);
    }
    if (box.x1 >= 0) {
      atomicMax(acc + 4 * b + 0, W - box.x0);
      atomicMax(acc + 4 * b + 1, box.x1 + 1);
      atomicMax(acc + 4 * b + 2, H - box.y0);
      atomicMax(acc + 4 * b + 3, box.y1 + 1);
    }
  }
}

// The accumulators' zeros: a kernel, so that a captured call is kernel nodes only.
__global__ void k_fundus_box_init(int32_t* __restrict__ acc, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) acc[i] = 0;
}

// acc -> (x_min, x_max, y_min, y_max) in place, with the fallback to the whole image
__global__ void k_fundus_box_finalize(FundusImages im, int n, int32_t* __restrict__ boxes) {
  const int b = threadIdx.x;
  if (b >= n) return;
  const int H = im.H[b], W = im.W[b];
  int32_t* a = boxes + 4 * b;
  int x0 = W - a[0], x1 = a[1] - 1, y0 = H - a[2], y1 = a[3] - 1;
  if (a[1] == 0 || x0 == x1 || y0 == y1) x0 = 0, x1 = W, y0 = 0, y1 = H;
  a[0] = x0, a[1] = x1, a[2] = y0, a[3] = y1;
}

// ---------------------------------------------------------------------------------------------
// crop -> resize -> pad -> normalise: one thread per output pixel, x fastest
// ---------------------------------------------------------------------------------------------

constexpr int kResizeThreads = 256;
constexpr int kCoefBits = 11;  // OpenCV's INTER_RESIZE_COEF_BITS

struct FundusNorm {
  float m[3], r[3];
};

// One axis of the 8-bit INTER_LINEAR resize: destination index d -> the first source index and
// the two coefficients (sum 2048). sc = 1.0 / (dst / src) in double.
__device__ __forceinline__ void linear_tap(int d, double sc, int src, int& s, int& a0, int& a1) {
#pragma clang fp contract(off)
  float f = (float)((d + 0.5) * sc - 0.5);
  int i = (int)floorf(f);
  f -= (float)i;
  if (i < 0) i = 0, f = 0.f;
  if (i >= src - 1) i = src - 1, f = 0.f;
  s = i;
  a0 = (int)rintf((1.f - f) * (float)(1 << kCoefBits));
  a1 = (int)rintf(f * (float)(1 << kCoefBits));
}

// INTER_NEAREST: min(floor(d * sc), src - 1)
__device__ __forceinline__ int nearest_tap(int d, double sc, int src) {
  return min((int)floor(d * sc), src - 1);
}

template <bool F32, bool U8, bool MASK>
__global__ __launch_bounds__(kResizeThreads) void k_fundus_resize(
    FundusImages im, const int32_t* __restrict__ boxes, int S, FundusNorm nm,
    float* __restrict__ out, uint8_t* __restrict__ out_u8, uint8_t* __restrict__ out_mask,
    int32_t* __restrict__ geom) {
  __shared__ int s_g[8];     // x_min, y_min, w, h, new_w, new_h, pad_left, pad_top
  __shared__ double s_sc[2];  // the x and y source steps
  const int b = blockIdx.y;
  const int H = im.H[b], W = im.W[b];
  if (threadIdx.x == 0) {
#pragma clang fp contract(off)
    const int32_t* bx = boxes + 4 * b;
    // clamped into the image: whatever boxes holds, no read leaves the image
    const int x0 = min(max(bx[0], 0), W - 1), x1 = min(max(bx[1], x0 + 1), W);
    const int y0 = min(max(bx[2], 0), H - 1), y1 = min(max(bx[3], y0 + 1), H);
    const int w = x1 - x0, h = y1 - y0;
    const double scale = (double)S / (double)max(h, w);
    const int nw = max(1, (int)rint(w * scale)), nh = max(1, (int)rint(h * scale));
    s_g[0] = x0, s_g[1] = y0, s_g[2] = w, s_g[3] = h, s_g[4] = nw, s_g[5] = nh;
    s_g[6] = (S - nw) / 2, s_g[7] = (S - nh) / 2;
    s_sc[0] = 1.0 / ((double)nw / (double)w);
    s_sc[1] = 1.0 / ((double)nh / (double)h);
    if (geom && blockIdx.x == 0)
      for (int k = 0; k < 8; ++k) geom[8 * b + k] = s_g[k];
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kResizeThreads + threadIdx.x;
  if (i >= (int64_t)S * S) return;
  const int dy = (int)(i / S), dx = (int)(i - (int64_t)dy * S);
  const int x0 = s_g[0], y0 = s_g[1], w = s_g[2], h = s_g[3];
  const int rx = dx - s_g[6], ry = dy - s_g[7];
  int v[3] = {0, 0, 0};
  int label = 0;
  if (rx >= 0 && rx < s_g[4] && ry >= 0 && ry < s_g[5]) {
    int sx, a0, a1, sy, b0, b1;
    linear_tap(rx, s_sc[0], w, sx, a0, a1);
    linear_tap(ry, s_sc[1], h, sy, b0, b1);
    const int sx1 = min(sx + 1, w - 1), sy1 = min(sy + 1, h - 1);
    const uint8_t* __restrict__ r0 = im.img[b] + ((int64_t)(y0 + sy) * W + x0) * 3;
    const uint8_t* __restrict__ r1 = im.img[b] + ((int64_t)(y0 + sy1) * W + x0) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int t0 = r0[3 * sx + c] * a0 + r0[3 * sx1 + c] * a1;
      const int t1 = r1[3 * sx + c] * a0 + r1[3 * sx1 + c] * a1;
      v[c] = (((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2;
    }
    if constexpr (MASK) {
      const int mx = nearest_tap(rx, s_sc[0], w), my = nearest_tap(ry, s_sc[1], h);
      label = im.mask[b][(int64_t)(y0 + my) * W + x0 + mx];
    }
  }
  if constexpr (F32) {
    float* o = out + (int64_t)b * 3 * S * S + i;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[(int64_t)c * S * S] = ((float)v[c] - nm.m[c]) * nm.r[c];
  }
  if constexpr (U8) {
    uint8_t* o = out_u8 + ((int64_t)b * S * S + i) * 3;
    o[0] = (uint8_t)v[0], o[1] = (uint8_t)v[1], o[2] = (uint8_t)v[2];
  }
  if constexpr (MASK) out_mask[(int64_t)b * S * S + i] = (uint8_t)label;
}

// The tables' checks shared by the two entries.
bool tables_ok(int batch, const uint8_t* const* images, const uint8_t* const* masks,
               const int* heights, const int* widths) {
  if (batch < 1 || !images || !heights || !widths) return false;
  for (int b = 0; b < batch; ++b) {
    if (!images[b] || (masks && !masks[b])) return false;
    if (heights[b] < 2 || heights[b] > LGNN_FUNDUS_MAX_SIDE || widths[b] < 2 ||
        widths[b] > LGNN_FUNDUS_MAX_SIDE)
      return false;
  }
  return true;
}

FundusImages pack(int at, int n, const uint8_t* const* images, const uint8_t* const* masks,
                  const int* heights, const int* widths) {
  FundusImages im = {};
  for (int k = 0; k < n; ++k) {
    im.img[k] = images[at + k];
    im.mask[k] = masks ? masks[at + k] : nullptr;
    im.H[k] = heights[at + k];
    im.W[k] = widths[at + k];
  }
  return im;
}

}  // namespace

extern "C" int lgnn_fundus_bbox_share(int height, int width) {
  if (height < 2 || height > LGNN_FUNDUS_MAX_SIDE || width < 2 || width > LGNN_FUNDUS_MAX_SIDE)
    return 0;
  int workgroups;
  return box_share(height, width, &workgroups);
}

extern "C" int lgnn_fundus_bbox(int batch, const uint8_t* const* images, const int* heights,
                                const int* widths, float threshold, int32_t* boxes,
                                void* stream) {
  if (!tables_ok(batch, images, nullptr, heights, widths) || !boxes) return LGNN_EINVAL;
  // red > threshold on integers: red >= the smallest integer above it (256: nothing is lit)
  const unsigned ti = std::isnan(threshold) || threshold >= 255.f ? 256u
                      : threshold < 0.f                           ? 0u
                                        : (unsigned)std::floor(threshold) + 1u;
  const hipStream_t s = as_stream(stream);
  enqueue(k_fundus_box_init, dim3((unsigned)((4 * (int64_t)batch + 255) / 256)), dim3(256), s,
          boxes, 4 * batch);
  for (int at = 0; at < batch; at += LGNN_FUNDUS_MAX_IMAGES) {
    const int n = std::min(batch - at, LGNN_FUNDUS_MAX_IMAGES);
    const FundusImages im = pack(at, n, images, nullptr, heights, widths);
    int most = 1;
    for (int k = 0; k < n; ++k) {
      int workgroups;
      box_share(im.H[k], im.W[k], &workgroups);
      most = std::max(most, workgroups);
    }
    enqueue(k_fundus_box, dim3((unsigned)most, (unsigned)n), dim3(kBoxThreads), s, im, ti,
            boxes + 4 * at);
    enqueue(k_fundus_box_finalize, dim3(1), dim3(64), s, im, n, boxes + 4 * at);
  }
  return last_error();
}

extern "C" int lgnn_fundus_preprocess(int batch, const uint8_t* const* images,
                                      const uint8_t* const* masks, const int* heights,
                                      const int* widths, const int32_t* boxes, int size,
                                      double mean0, double mean1, double mean2, double std0,
                                      double std1, double std2, float* out, uint8_t* out_u8,
                                      uint8_t* out_mask, int32_t* geom, void* stream) {
  if (!tables_ok(batch, images, masks, heights, widths) || !boxes) return LGNN_EINVAL;
  if (size < 2 || size > LGNN_FUNDUS_MAX_SIDE || (!out && !out_u8) || (out_mask && !masks))
    return LGNN_EINVAL;
  const double mean[3] = {mean0, mean1, mean2}, stdv[3] = {std0, std1, std2};
  FundusNorm nm;
  for (int c = 0; c < 3; ++c) {
    if (!std::isfinite(mean[c]) || !std::isfinite(stdv[c]) || !(stdv[c] > 0.0))
      return LGNN_EINVAL;
    nm.m[c] = (float)(mean[c] * 255.0);
    nm.r[c] = (float)(1.0 / (stdv[c] * 255.0));
  }
  const hipStream_t s = as_stream(stream);
  const unsigned blocks = (unsigned)(((int64_t)size * size + kResizeThreads - 1) / kResizeThreads);
  for (int at = 0; at < batch; at += LGNN_FUNDUS_MAX_IMAGES) {
    const int n = std::min(batch - at, LGNN_FUNDUS_MAX_IMAGES);
    const FundusImages im = pack(at, n, images, out_mask ? masks : nullptr, heights, widths);
    const int64_t px = (int64_t)at * size * size;
    one_of<false, true>(out != nullptr, [&](auto F32) {
      one_of<false, true>(out_u8 != nullptr, [&](auto U8) {
        one_of<false, true>(out_mask != nullptr, [&](auto MASK) {
          constexpr bool f32 = decltype(F32)::value, u8 = decltype(U8)::value;
          constexpr bool mask = decltype(MASK)::value;
          if constexpr (f32 || u8)
            enqueue(k_fundus_resize<f32, u8, mask>, dim3(blocks, (unsigned)n),
                    dim3(kResizeThreads), s, im, boxes + 4 * at, size, nm,
                    out ? out + 3 * px : nullptr, out_u8 ? out_u8 + 3 * px : nullptr,
                    out_mask ? out_mask + px : nullptr, geom ? geom + 8 * at : nullptr);
        });
      });
    });
  }
  return last_error();
}
