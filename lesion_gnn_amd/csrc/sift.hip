// SIFT nodes (reference src/lesion_gnn/datasets/nodes/sift.py:17-70: cv2.SIFT_create(nfeatures,
// contrastThreshold = 0, sigma).detectAndCompute) for a batch of images of one size, on the
// device: OpenCV's algorithm with its default nOctaveLayers = 3 and edgeThreshold = 10, restated
// (tests/sift_ref.py is the float64 statement the tests hold this file to).
//
//   lgnn_sift_pyramid      gray, doubled base, Gaussian and DoG levels of every octave: fp32, one
//                          workgroup per 64 x 64 tile with its halo in LDS, rows and columns in one
//                          launch, the DoG level written from the same launch, the image index a
//                          grid dimension.
//   lgnn_sift_count /      26-neighbour extrema, one wave per DoG row: counted, scanned, then
//   lgnn_sift_candidates   written at their offsets, so the list is in (image, octave, layer, row,
//                          column) order without a sort and without an atomic append.
//   lgnn_sift_keypoints /  refinement, orientation peaks, duplicate removal, the response cut and
//   lgnn_sift_gather       the output order; the caller reads node_ptr between the two.
//   lgnn_sift_descriptors  the 4 x 4 x 8 histograms.
//
// Everything after the pyramid is float64 on the fp32 levels, in the operation order of the
// oracle and without FMA contraction: these are a few thousand small problems that each end in a
// discrete decision (move or stay, keep or reject, which bin, which peak, which integer), and in
// float64 the device takes the decisions the oracle takes. No float atomics anywhere: two runs
// give the same bits. Every loop is bounded and every write is checked against its capacity.
#include <math.h>

#include "launch.h"
#include "wg.h"

#pragma clang fp contract(off)

namespace {

constexpr int kLayers = 3;                 // nOctaveLayers
constexpr int kLevels = kLayers + 3;       // Gaussian levels per octave
constexpr int kDogs = kLayers + 2;         // DoG levels per octave
constexpr int kBorder = 5;
constexpr int kSteps = 5;
constexpr int kOriBins = 36;
constexpr int kMaxPeaks = LGNN_SIFT_MAX_PEAKS;
constexpr int kMaxOct = LGNN_SIFT_MAX_OCTAVES;
constexpr int kMaxRadius = LGNN_SIFT_MAX_RADIUS;
constexpr int kTile = 64;
constexpr int kIn = kTile + 2 * kMaxRadius;
constexpr int kD = 4, kN = 8;              // descriptor grid
constexpr int kHist = (kD + 2) * (kD + 2) * (kN + 2);
constexpr double kFltEps = 1.1920928955078125e-07;
constexpr double kSingular = 100.0 * 2.220446049250313e-16;
constexpr double kIntMax3 = 2147483647.0 / 3.0;
constexpr double kDeg = 180.0 / 3.141592653589793;
constexpr double kRad = 3.141592653589793 / 180.0;

struct Octaves {
  int n;
  int h[kMaxOct], w[kMaxOct];
  int rowbase[kMaxOct + 1];       // first scan row of the octave within one image: 3 * sum h
  int64_t goff[kMaxOct + 1];      // first float of the octave in the Gaussian buffer
  int64_t doff[kMaxOct + 1];      // ... in the DoG buffer
};

struct Taps {
  int r;
  float w[2 * kMaxRadius + 1];
};

// ---- host: sizes ------------------------------------------------------------------------------

bool dims_ok(int batch, int height, int width) {
  if (batch < 1 || batch > 65535 || height < 2 || width < 2) return false;  // a grid dimension
  return (int64_t)batch * kLevels * 4 * height * width < ((int64_t)1 << 31);
}

Octaves octaves(int batch, int height, int width) {
  Octaves oc = {};
  int h = 2 * height, w = 2 * width;
  const int n = (int)rint(log((double)(h < w ? h : w)) / log(2.0) - 2.0) + 1;
  oc.rowbase[0] = 0;
  oc.goff[0] = oc.doff[0] = 0;
  for (int o = 0; o < n && o < kMaxOct; ++o) {
    if ((h < w ? h : w) <= 2 * kBorder) break;  // no pixel inside the border
    oc.h[o] = h;
    oc.w[o] = w;
    oc.rowbase[o + 1] = oc.rowbase[o] + kLayers * h;
    oc.goff[o + 1] = oc.goff[o] + (int64_t)batch * kLevels * h * w;
    oc.doff[o + 1] = oc.doff[o] + (int64_t)batch * kDogs * h * w;
    oc.n = o + 1;
    h /= 2;
    w /= 2;
  }
  return oc;
}

int kernel_size(double sigma) { return (int)rint(8.0 * sigma + 1.0) | 1; }

bool make_taps(double sigma, Taps* t) {
  const int k = kernel_size(sigma), r = (k - 1) / 2;
  if (r > kMaxRadius) return false;
  double w[2 * kMaxRadius + 1], sum = 0.0;
  for (int i = 0; i < k; ++i) {
    const double x = i - r;
    w[i] = exp(-(x * x) / (2.0 * sigma * sigma));
    sum += w[i];
  }
  t->r = r;
  for (int i = 0; i < k; ++i) t->w[i] = (float)(w[i] / sum);
  return true;
}

double base_sigma(double sigma) {
  const double v = sigma * sigma - 1.0;  // the doubled image is assumed blurred by 2 * 0.5
  return sqrt(v > 0.01 ? v : 0.01);
}

// the blur that takes level i - 1 to level i, i = 1..5
double level_sigma(double sigma, int i) {
  const double k = pow(2.0, 1.0 / kLayers);
  const double prev = sigma * pow(k, i - 1), total = prev * k;
  return sqrt(total * total - prev * prev);
}

bool sigma_ok(double sigma) {
  if (!(sigma > 0.0) || !(sigma < 1e6)) return false;
  Taps t;
  if (!make_taps(base_sigma(sigma), &t)) return false;
  for (int i = 1; i < kLevels; ++i)
    if (!make_taps(level_sigma(sigma, i), &t)) return false;
  return true;
}

// ---- pyramid ----------------------------------------------------------------------------------

// BORDER_REFLECT_101, applied until the index is inside: the radius may exceed the side
__device__ __forceinline__ int reflect101(int i, int n) {
  for (int k = 0; k < 8 && (i < 0 || i >= n); ++k) i = i < 0 ? -i : 2 * (n - 1) - i;
  return i < 0 ? 0 : i >= n ? n - 1 : i;
}

// The RGB array goes through a conversion that assumes BGR (the reference calls cvtColor(BGR2RGB)
// and then hands the result to SIFT, which converts with BGR2GRAY): channel 0, red, gets the
// 0.114 weight. The quirk is the reference's and is kept.
__global__ __launch_bounds__(256) void k_gray(const uint8_t* __restrict__ img, int64_t n,
                                              int channels, uint8_t* __restrict__ gray) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (channels == 1) {
    gray[i] = img[i];
    return;
  }
  const int c0 = img[3 * i], c1 = img[3 * i + 1], c2 = img[3 * i + 2];
  gray[i] = (uint8_t)((c0 * 1868 + c1 * 9617 + c2 * 4899 + 8192) >> 14);
}

// pixel (y, x) of the doubled image: bilinear at (d + 0.5) / 2 - 0.5, indices clamped. The
// weights are 0.25 and 0.75 and the values multiples of 1/16 below 256: exact in fp32.
__device__ __forceinline__ float doubled(const uint8_t* g, int sh, int sw, int y, int x) {
  const int ys = (y + 1) / 2 - 1, xs = (x + 1) / 2 - 1;  // floor((d + 0.5) / 2 - 0.5)
  const float fy = (y & 1) ? 0.25f : 0.75f, fx = (x & 1) ? 0.25f : 0.75f;
  const int y0 = ys < 0 ? 0 : ys, y1 = ys + 1 > sh - 1 ? sh - 1 : ys + 1;
  const int x0 = xs < 0 ? 0 : xs, x1 = xs + 1 > sw - 1 ? sw - 1 : xs + 1;
  const float a = g[(int64_t)y0 * sw + x0], b = g[(int64_t)y0 * sw + x1];
  const float c = g[(int64_t)y1 * sw + x0], d = g[(int64_t)y1 * sw + x1];
  const float top = a * (1.f - fx) + b * fx, bot = c * (1.f - fx) + d * fx;
  return top * (1.f - fy) + bot * fy;
}

// One separable Gaussian blur of one level of every image: workgroup (tile x, tile y, image).
// The tile and its halo are staged in LDS (reflect-101 at the image's edge), the row pass writes
// a second LDS array, the column pass the output; dog (nullable) = output - input.
// GRAY: the source is the uint8 gray image, doubled as it is staged.
template <bool GRAY>
__global__ __launch_bounds__(256) void k_blur(const void* __restrict__ src_, int64_t src_stride,
                                              float* __restrict__ dst, int64_t dst_stride,
                                              float* __restrict__ dog, int64_t dog_stride, int h,
                                              int w, Taps taps) {
#pragma clang fp contract(fast)
  __shared__ float s_in[kIn * kIn];
  __shared__ float s_mid[kIn * kTile];
  const int r = taps.r, tw = kTile + 2 * r;
  const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile, b = blockIdx.z;
  const int tid = threadIdx.x;
  const float* srcf = GRAY ? nullptr : (const float*)src_ + b * src_stride;
  const uint8_t* srcg = GRAY ? (const uint8_t*)src_ + b * src_stride : nullptr;
  for (int i = tid; i < tw * tw; i += 256) {
    const int ty = i / tw, tx = i - ty * tw;
    const int gy = reflect101(y0 - r + ty, h), gx = reflect101(x0 - r + tx, w);
    s_in[ty * kIn + tx] = GRAY ? doubled(srcg, h / 2, w / 2, gy, gx) : srcf[(int64_t)gy * w + gx];
  }
  __syncthreads();
  for (int i = tid; i < tw * kTile; i += 256) {
    const int ty = i / kTile, x = i - ty * kTile;
    float acc = 0.f;
    for (int t = 0; t <= 2 * r; ++t) acc += taps.w[t] * s_in[ty * kIn + x + t];
    s_mid[ty * kTile + x] = acc;
  }
  __syncthreads();
  for (int i = tid; i < kTile * kTile; i += 256) {
    const int y = i / kTile, x = i - y * kTile;
    if (y0 + y >= h || x0 + x >= w) continue;
    float acc = 0.f;
    for (int t = 0; t <= 2 * r; ++t) acc += taps.w[t] * s_mid[(y + t) * kTile + x];
    const int64_t at = (int64_t)(y0 + y) * w + x0 + x;
    dst[b * dst_stride + at] = acc;
    if (dog) dog[b * dog_stride + at] = acc - s_in[(y + r) * kIn + x + r];
  }
}

// level 0 of the next octave: level 3 sampled at [2i, 2j]
__global__ __launch_bounds__(256) void k_down(const float* __restrict__ src, int64_t src_stride,
                                              int sw, float* __restrict__ dst,
                                              int64_t dst_stride, int h, int w) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= h * w) return;
  const int y = i / w, x = i - y * w;
  dst[b * dst_stride + i] = src[b * src_stride + (int64_t)(2 * y) * sw + 2 * x];
}

// ---- candidates -------------------------------------------------------------------------------

struct Row {
  int b, o, layer, r;
};

__device__ __forceinline__ Row decode_row(const Octaves& oc, int row) {
  const int per = oc.rowbase[oc.n];
  Row q;
  q.b = row / per;
  const int rem = row - q.b * per;
  q.o = 0;
  for (int o = 1; o < oc.n; ++o)
    if (rem >= oc.rowbase[o]) q.o = o;
  const int in = rem - oc.rowbase[q.o];
  q.layer = in / oc.h[q.o] + 1;
  q.r = in - (q.layer - 1) * oc.h[q.o];
  return q;
}

// v > 0 and >= all 26 neighbours, or v < 0 and <= all 26; d points at DoG level 0 of the image's
// octave, (r, c) lies inside the border and layer in 1..3
__device__ __forceinline__ bool is_extremum(const float* d, int h, int w, int layer, int r,
                                            int c) {
  const int64_t plane = (int64_t)h * w;
  const float v = d[layer * plane + (int64_t)r * w + c];
  if (v == 0.f) return false;
  bool hi = true, lo = true;
  for (int dl = -1; dl <= 1; ++dl)
    for (int dr = -1; dr <= 1; ++dr)
      for (int dc = -1; dc <= 1; ++dc) {
        const float nb = d[(layer + dl) * plane + (int64_t)(r + dr) * w + c + dc];
        hi = hi && v >= nb;
        lo = lo && v <= nb;
      }
  return v > 0.f ? hi : lo;
}

// One wave per scan row. WRITE = false: counts[row] = the row's candidates. WRITE = true: the
// candidates go to cand[row_ptr[row] ...] in column order (capacity checked).
template <bool WRITE>
__global__ __launch_bounds__(256) void k_extrema(const float* __restrict__ dog, Octaves oc,
                                                 int rows, int32_t* __restrict__ counts,
                                                 const int32_t* __restrict__ row_ptr,
                                                 int32_t* __restrict__ cand, int capacity) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const Row q = decode_row(oc, row);
  const int h = oc.h[q.o], w = oc.w[q.o];
  int total = 0;
  if (q.r >= kBorder && q.r < h - kBorder) {
    const float* d = dog + oc.doff[q.o] + (int64_t)q.b * kDogs * h * w;
    const int base = WRITE ? row_ptr[row] : 0;
    for (int c0 = kBorder; c0 < w - kBorder; c0 += 64) {
      const int c = c0 + lane;
      const bool e = c < w - kBorder && is_extremum(d, h, w, q.layer, q.r, c);
      const unsigned long long m = __ballot(e);
      if (WRITE && e) {
        const int at = base + total + __popcll(m & ((1ull << lane) - 1ull));
        if (at >= 0 && at < capacity) {
          int32_t* p = cand + (int64_t)at * 5;
          p[0] = q.b, p[1] = q.o, p[2] = q.layer, p[3] = q.r, p[4] = c;
        }
      }
      total += __popcll(m);
    }
  }
  if (!WRITE && lane == 0) counts[row] = total;
}

// ---- refinement -------------------------------------------------------------------------------

struct Refined {  // one per candidate
  int valid, o, layer, r, c;
  float x, y, size, response;  // in the doubled image's pixels, rounded as cv::KeyPoint holds them
};

// Gaussian elimination with partial pivoting (OpenCV's LU); a singular system gives zeros
__device__ void solve3(double A[3][3], double b[3], double x[3]) {
  x[0] = x[1] = x[2] = 0.0;
  for (int i = 0; i < 3; ++i) {
    int k = i;
    for (int j = i + 1; j < 3; ++j)
      if (fabs(A[j][i]) > fabs(A[k][i])) k = j;
    if (fabs(A[k][i]) < kSingular) return;
    if (k != i) {
      for (int c = 0; c < 3; ++c) {
        const double t = A[i][c];
        A[i][c] = A[k][c];
        A[k][c] = t;
      }
      const double t = b[i];
      b[i] = b[k];
      b[k] = t;
    }
    const double d = -1.0 / A[i][i];
    for (int j = i + 1; j < 3; ++j) {
      const double alpha = A[j][i] * d;
      for (int c = i + 1; c < 3; ++c) A[j][c] += alpha * A[i][c];
      b[j] += alpha * b[i];
    }
  }
  for (int i = 2; i >= 0; --i) {
    double s = b[i];
    for (int c = i + 1; c < 3; ++c) s -= A[i][c] * x[c];
    x[i] = s / A[i][i];
  }
}

struct Derivs {
  double dD[3], dxx, dyy, dss, dxy, dxs, dys, v;
};

__device__ Derivs derivs(const float* d, int h, int w, int layer, int r, int c) {
  const int64_t plane = (int64_t)h * w;
  const float* img = d + layer * plane;
  const float* prv = img - plane;
  const float* nxt = img + plane;
#define AT(p, rr, cc) ((double)(p)[(int64_t)(rr) * w + (cc)])
  const double scale = 1.0 / 255.0, ds = scale * 0.5, cs = scale * 0.25;
  Derivs q;
  q.v = AT(img, r, c);
  q.dD[0] = (AT(img, r, c + 1) - AT(img, r, c - 1)) * ds;
  q.dD[1] = (AT(img, r + 1, c) - AT(img, r - 1, c)) * ds;
  q.dD[2] = (AT(nxt, r, c) - AT(prv, r, c)) * ds;
  const double v2 = q.v * 2.0;
  q.dxx = (AT(img, r, c + 1) + AT(img, r, c - 1) - v2) * scale;
  q.dyy = (AT(img, r + 1, c) + AT(img, r - 1, c) - v2) * scale;
  q.dss = (AT(nxt, r, c) + AT(prv, r, c) - v2) * scale;
  q.dxy = (AT(img, r + 1, c + 1) - AT(img, r + 1, c - 1) - AT(img, r - 1, c + 1) +
           AT(img, r - 1, c - 1)) * cs;
  q.dxs = (AT(nxt, r, c + 1) - AT(nxt, r, c - 1) - AT(prv, r, c + 1) + AT(prv, r, c - 1)) * cs;
  q.dys = (AT(nxt, r + 1, c) - AT(nxt, r - 1, c) - AT(prv, r + 1, c) + AT(prv, r - 1, c)) * cs;
#undef AT
  return q;
}

// OpenCV's adjustLocalExtrema, one thread per candidate
__global__ __launch_bounds__(64) void k_refine(const float* __restrict__ dog, Octaves oc,
                                               int batch, double sigma,
                                               const int32_t* __restrict__ cand, int n,
                                               Refined* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  Refined q = {};
  const int b = cand[5 * i], o = cand[5 * i + 1];
  int layer = cand[5 * i + 2], r = cand[5 * i + 3], c = cand[5 * i + 4];
  out[i] = q;
  if (b < 0 || b >= batch || o < 0 || o >= oc.n) return;
  const int h = oc.h[o], w = oc.w[o];
  if (layer < 1 || layer > kLayers || r < kBorder || r >= h - kBorder || c < kBorder ||
      c >= w - kBorder)
    return;
  const float* d = dog + oc.doff[o] + (int64_t)b * kDogs * h * w;
  double xi = 0.0, xr = 0.0, xc = 0.0;
  bool ok = false;
  for (int step = 0; step < kSteps; ++step) {
    const Derivs g = derivs(d, h, w, layer, r, c);
    double A[3][3] = {{g.dxx, g.dxy, g.dxs}, {g.dxy, g.dyy, g.dys}, {g.dxs, g.dys, g.dss}};
    double rhs[3] = {g.dD[0], g.dD[1], g.dD[2]}, X[3];
    solve3(A, rhs, X);
    xc = -X[0], xr = -X[1], xi = -X[2];
    if (fabs(xi) < 0.5 && fabs(xr) < 0.5 && fabs(xc) < 0.5) {
      ok = true;
      break;
    }
    if (!(fabs(xi) <= kIntMax3 && fabs(xr) <= kIntMax3 && fabs(xc) <= kIntMax3)) break;
    c += (int)rint(xc);
    r += (int)rint(xr);
    layer += (int)rint(xi);
    if (layer < 1 || layer > kLayers || c < kBorder || c >= w - kBorder || r < kBorder ||
        r >= h - kBorder)
      break;
  }
  if (!ok) return;
  const Derivs g = derivs(d, h, w, layer, r, c);
  const double t = g.dD[0] * xc + g.dD[1] * xr + g.dD[2] * xi;
  const double contr = g.v * (1.0 / 255.0) + t * 0.5;
  const double tr = g.dxx + g.dyy, det = g.dxx * g.dyy - g.dxy * g.dxy;
  if (det <= 0.0 || tr * tr * 10.0 >= 121.0 * det) return;
  const double s = (double)(1 << o);
  q.valid = 1, q.o = o, q.layer = layer, q.r = r, q.c = c;
  q.x = (float)((c + xc) * s);
  q.y = (float)((r + xr) * s);
  q.size = (float)(sigma * pow(2.0, (layer + xi) / 3.0) * s * 2.0);
  q.response = (float)fabs(contr);
  out[i] = q;
}

// ---- orientation ------------------------------------------------------------------------------

// The 36-bin index of a gradient. |dx| == |dy| lies exactly between two bins and goes to the lower
// one by this branch; no other bin boundary has a rational tangent, so fp32 pixel differences
// reach no other exact tie.
__device__ __forceinline__ int gradient_bin(double dx, double dy) {
  if (fabs(dx) == fabs(dy)) {
    if (dx == 0.0) return 0;
    return dy > 0.0 ? (dx > 0.0 ? 4 : 13) : (dx < 0.0 ? 22 : 31);
  }
  double ori = atan2(dy, dx) * kDeg;
  if (ori < 0.0) ori += 360.0;
  const int bin = (int)rint(ori / 10.0);
  return bin >= kOriBins ? bin - kOriBins : bin;
}

// One wave per candidate: lane l takes the samples l, l + 64, ... of the window in raster order
// into its own column of the LDS histogram; the columns are summed in lane order.
__global__ __launch_bounds__(64) void k_orient(const float* __restrict__ gauss, Octaves oc,
                                               int batch, const int32_t* __restrict__ cand,
                                               const Refined* __restrict__ ref, int n,
                                               int32_t* __restrict__ npk,
                                               float* __restrict__ angles) {
  __shared__ double s_hist[kOriBins][64];
  __shared__ double s_raw[kOriBins];
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= n) return;
  const Refined q = ref[i];
  const int b = cand[5 * i];
  if (!q.valid || b < 0 || b >= batch) {
    if (lane == 0) npk[i] = 0;
    return;
  }
  const int h = oc.h[q.o], w = oc.w[q.o];
  const float* img = gauss + oc.goff[q.o] + ((int64_t)b * kLevels + q.layer) * h * w;
  const double scl = (double)q.size * 0.5 / (double)(1 << q.o);
  int radius = (int)rint(4.5 * scl);
  radius = radius < 0 ? 0 : radius > h + w ? h + w : radius;
  const double sig = 1.5 * scl, expf_scale = -1.0 / (2.0 * sig * sig);
  for (int k = 0; k < kOriBins; ++k) s_hist[k][lane] = 0.0;
  const int side = 2 * radius + 1;
  for (int s = lane; s < side * side; s += 64) {
    const int di = s / side - radius, dj = s % side - radius;
    const int y = q.r + di, x = q.c + dj;
    if (y <= 0 || y >= h - 1 || x <= 0 || x >= w - 1) continue;
    const double dx = (double)img[(int64_t)y * w + x + 1] - (double)img[(int64_t)y * w + x - 1];
    const double dy = (double)img[(int64_t)(y - 1) * w + x] - (double)img[(int64_t)(y + 1) * w + x];
    const double wgt = exp((double)(di * di + dj * dj) * expf_scale);
    s_hist[gradient_bin(dx, dy)][lane] += wgt * sqrt(dx * dx + dy * dy);
  }
  __syncthreads();
  if (lane < kOriBins) {
    double acc = 0.0;
    for (int l = 0; l < 64; ++l) acc += s_hist[lane][l];
    s_raw[lane] = acc;
  }
  __syncthreads();
  if (lane != 0) return;
  double hist[kOriBins], mx = 0.0;
  for (int k = 0; k < kOriBins; ++k) {
    const int m2 = (k + kOriBins - 2) % kOriBins, m1 = (k + kOriBins - 1) % kOriBins;
    const int p1 = (k + 1) % kOriBins, p2 = (k + 2) % kOriBins;
    hist[k] = (s_raw[m2] + s_raw[p2]) * (1.0 / 16.0) + (s_raw[m1] + s_raw[p1]) * (4.0 / 16.0) +
              s_raw[k] * (6.0 / 16.0);
    mx = k == 0 || hist[k] > mx ? hist[k] : mx;
  }
  const double thr = mx * 0.8;
  int count = 0;
  for (int j = 0; j < kOriBins; ++j) {
    const double left = hist[j > 0 ? j - 1 : kOriBins - 1];
    const double right = hist[j < kOriBins - 1 ? j + 1 : 0];
    if (hist[j] > left && hist[j] > right && hist[j] >= thr && count < kMaxPeaks) {
      double bin = j + 0.5 * (left - right) / (left - 2.0 * hist[j] + right);
      bin = bin < 0.0 ? kOriBins + bin : bin >= kOriBins ? bin - kOriBins : bin;
      float angle = (float)(360.0 - 10.0 * bin);
      if (fabs((double)angle - 360.0) < kFltEps) angle = 0.f;
      angles[(int64_t)i * kMaxPeaks + count++] = angle;
    }
  }
  npk[i] = count;
}

// ---- duplicates, selection, order -------------------------------------------------------------

struct Keypoint {  // one per orientation peak, in canonical order
  float x, y, size, angle, response;
  int b, o, layer;
};

// image b's candidates are [cstart[b], cstart[b + 1]), its keypoints [kstart[b], kstart[b + 1])
__global__ void k_ranges(const int32_t* __restrict__ cand, int n, const int32_t* __restrict__ koff,
                         int batch, int32_t* __restrict__ kstart, float* __restrict__ thr,
                         int32_t* __restrict__ kept) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b > batch) return;
  int lo = 0, hi = n;  // the first candidate of an image >= b
  for (int k = 0; k < 32 && lo < hi; ++k) {
    const int mid = lo + (hi - lo) / 2;
    if (cand[5 * mid] < b) lo = mid + 1; else hi = mid;
  }
  kstart[b] = koff[lo];
  if (b < batch) thr[b] = -INFINITY, kept[b] = 0;
}

__global__ __launch_bounds__(64) void k_flatten(const int32_t* __restrict__ cand,
                                                const Refined* __restrict__ ref,
                                                const int32_t* __restrict__ npk,
                                                const int32_t* __restrict__ koff,
                                                const float* __restrict__ angles, int n,
                                                int capacity, Keypoint* __restrict__ kp) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const Refined q = ref[i];
  for (int p = 0; p < npk[i] && p < kMaxPeaks; ++p) {
    const int at = koff[i] + p;
    if (at < 0 || at >= capacity) return;
    kp[at] = Keypoint{q.x, q.y, q.size, angles[(int64_t)i * kMaxPeaks + p], q.response,
                      cand[5 * i], q.o, q.layer};
  }
}

// alive: no earlier keypoint of the image equals this one in (pt, size, angle). rank: its place
// among the image's alive keypoints by response descending, then canonical order. Both compare
// every keypoint with its image's others; the others pass through LDS 64 at a time, so a wave
// makes one coalesced load per 64 comparisons instead of a dependent load per comparison.
__global__ __launch_bounds__(64) void k_dedupe(const Keypoint* __restrict__ kp,
                                               const int32_t* __restrict__ kstart, int batch,
                                               int total_cap, int32_t* __restrict__ alive) {
  __shared__ float s_x[64], s_y[64], s_size[64], s_angle[64];
  __shared__ int s_first;
  const int total = kstart[batch] < total_cap ? kstart[batch] : total_cap;
  const int j0 = blockIdx.x * 64, lane = threadIdx.x, j = j0 + lane;
  if (j0 >= total) return;
  const bool on = j < total;
  Keypoint q = {};
  if (on) q = kp[j];
  const int lo = on ? kstart[q.b] : total;  // the image's first keypoint
  if (lane == 0) s_first = total;
  __syncthreads();
  if (on) atomicMin(&s_first, lo);
  __syncthreads();
  int a = 1;
  for (int t0 = s_first < 0 ? 0 : s_first; t0 < j0 + 64 && t0 < total; t0 += 64) {
    if (t0 + lane < total) {
      const Keypoint t = kp[t0 + lane];
      s_x[lane] = t.x, s_y[lane] = t.y, s_size[lane] = t.size, s_angle[lane] = t.angle;
    }
    __syncthreads();
    const int n = total - t0 < 64 ? total - t0 : 64;
    for (int k = 0; k < n; ++k) {
      const int e = t0 + k;
      if (e >= lo && e < j && s_x[k] == q.x && s_y[k] == q.y && s_size[k] == q.size &&
          s_angle[k] == q.angle)
        a = 0;
    }
    __syncthreads();
  }
  if (on) alive[j] = a;
}

__global__ __launch_bounds__(64) void k_rank(const Keypoint* __restrict__ kp,
                                             const int32_t* __restrict__ kstart, int batch,
                                             int total_cap, const int32_t* __restrict__ alive,
                                             int num_keypoints, int32_t* __restrict__ rank,
                                             float* __restrict__ thr) {
  __shared__ float s_resp[64];
  __shared__ int s_first, s_last;
  const int total = kstart[batch] < total_cap ? kstart[batch] : total_cap;
  const int j0 = blockIdx.x * 64, lane = threadIdx.x, j = j0 + lane;
  if (j0 >= total) return;
  const bool on = j < total && alive[j];
  Keypoint q = {};
  if (on) q = kp[j];
  int lo = total, hi = 0;  // the image's keypoints
  if (on) lo = kstart[q.b], hi = kstart[q.b + 1] < total ? kstart[q.b + 1] : total;
  if (lane == 0) s_first = total, s_last = 0;
  __syncthreads();
  if (on) atomicMin(&s_first, lo), atomicMax(&s_last, hi);
  __syncthreads();
  int rk = 0;
  for (int t0 = s_first < 0 ? 0 : s_first; t0 < s_last; t0 += 64) {
    const int at = t0 + lane;
    // a dropped keypoint outranks nothing
    s_resp[lane] = at < total && alive[at] ? kp[at].response : -INFINITY;
    __syncthreads();
    const int n = s_last - t0 < 64 ? s_last - t0 : 64;
    for (int k = 0; k < n; ++k) {
      const int e = t0 + k;
      const float t = s_resp[k];
      rk += e >= lo && e < hi && (t > q.response || (t == q.response && e < j));
    }
    __syncthreads();
  }
  if (j < total) rank[j] = on ? rk : -1;
  if (on && rk == num_keypoints - 1) thr[q.b] = q.response;  // the one keypoint of that rank
}

// keep every alive keypoint whose response reaches the num_keypoints-th largest (ties kept, as
// retainBest does); they are the ranks [0, kept[b])
__global__ __launch_bounds__(64) void k_keep(const Keypoint* __restrict__ kp,
                                             const int32_t* __restrict__ kstart, int batch,
                                             int total_cap, const int32_t* __restrict__ alive,
                                             const float* __restrict__ thr,
                                             int32_t* __restrict__ kept) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= kstart[batch] || j >= total_cap) return;
  if (alive[j] && kp[j].response >= thr[kp[j].b]) atomicAdd(kept + kp[j].b, 1);
}

// row node_ptr[b] + rank: pt and size halved for the doubled image (exact)
__global__ __launch_bounds__(64) void k_gather(const Keypoint* __restrict__ kp,
                                               const int32_t* __restrict__ kstart, int batch,
                                               int total_cap, const int32_t* __restrict__ alive,
                                               const int32_t* __restrict__ rank,
                                               const float* __restrict__ thr,
                                               const int64_t* __restrict__ node_ptr, int total,
                                               float* __restrict__ kf, int32_t* __restrict__ ki) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= kstart[batch] || j >= total_cap) return;
  const Keypoint q = kp[j];
  if (!alive[j] || !(q.response >= thr[q.b])) return;
  const int64_t row = node_ptr[q.b] + rank[j];
  if (rank[j] < 0 || row < 0 || row >= node_ptr[q.b + 1] || row >= total) return;
  float* f = kf + row * 5;
  f[0] = q.x * 0.5f, f[1] = q.y * 0.5f, f[2] = q.size * 0.5f, f[3] = q.angle, f[4] = q.response;
  int32_t* k = ki + row * 3;
  k[0] = q.b, k[1] = q.o, k[2] = q.layer;
}

// ---- descriptors ------------------------------------------------------------------------------

// OpenCV's calcSIFTDescriptor, one wave per keypoint. The window is taken 64 samples at a time in
// raster order: every lane forms one sample (rotation, gradient, weight: the transcendental
// part) and stages it in LDS; then lane (R, C) of the first 36, which owns the 10 orientation bins
// of spatial cell (R, C) of the (4 + 2) x (4 + 2) x (8 + 2) histogram, walks the 64 staged
// samples in order and adds the trilinear shares that fall into its cell. Every bin is summed in
// raster order by one lane: no atomics, the same bits every run and the order of the oracle.
__global__ __launch_bounds__(64) void k_descriptors(const float* __restrict__ gauss, Octaves oc,
                                                    int batch, const float* __restrict__ kf,
                                                    const int32_t* __restrict__ ki, int n,
                                                    float* __restrict__ out) {
  __shared__ double s_hist[kHist];
  __shared__ double s_mag[64], s_rb[64], s_cb[64], s_ob[64], s_scale;
  __shared__ int s_r0[64], s_c0[64], s_o0[64];
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= n) return;
  float* dst = out + (int64_t)i * (kD * kD * kN);
  dst[lane] = 0.f;
  dst[lane + 64] = 0.f;
  const int b = ki[3 * i], o = ki[3 * i + 1], layer = ki[3 * i + 2];
  if (b < 0 || b >= batch || o < 0 || o >= oc.n || layer < 0 || layer >= kLevels) return;
  const int h = oc.h[o], w = oc.w[o];
  const float* img = gauss + oc.goff[o] + ((int64_t)b * kLevels + layer) * h * w;
  // the halved fp32 values doubled and scaled by the octave: exact powers of two
  const double s = 2.0 / (double)(1 << o);
  const double x = (double)kf[5 * i] * s, y = (double)kf[5 * i + 1] * s;
  const double scl = (double)kf[5 * i + 2] * s * 0.5;
  double ori = 360.0 - (double)kf[5 * i + 3];
  if (fabs(ori - 360.0) < kFltEps) ori = 0.0;
  const double hist_width = 3.0 * scl;
  if (!(hist_width > 0.0) || !(fabs(x) < 1e9) || !(fabs(y) < 1e9) || !(fabs(ori) < 1e9)) return;
  const int px = (int)rint(x), py = (int)rint(y);
  double cos_t = cos(ori * kRad), sin_t = sin(ori * kRad);
  const double bins_per_deg = kN / 360.0, exp_scale = -1.0 / (kD * kD * 0.5);
  const double rad = hist_width * 1.4142135623730951 * (kD + 1) * 0.5;
  const int diag = (int)sqrt((double)h * h + (double)w * w);
  const int radius = rad < (double)diag ? (int)rint(rad) < diag ? (int)rint(rad) : diag : diag;
  cos_t /= hist_width;
  sin_t /= hist_width;
  for (int k = lane; k < kHist; k += 64) s_hist[k] = 0.0;
  const int64_t side = 2 * (int64_t)radius + 1, total = side * side;
  const int R = lane / (kD + 2) - 1, C = lane % (kD + 2) - 1;  // the cell of lanes 0..35
  for (int64_t first = 0; first < total; first += 64) {
    const int64_t at = first + lane;
    int r0 = -2;  // no sample
    if (at < total) {
      const int di = (int)(at / side) - radius, dj = (int)(at % side) - radius;
      const double c_rot = dj * cos_t - di * sin_t, r_rot = dj * sin_t + di * cos_t;
      double rbin = r_rot + kD / 2 - 0.5, cbin = c_rot + kD / 2 - 0.5;
      const int r = py + di, c = px + dj;
      if (rbin > -1.0 && rbin < kD && cbin > -1.0 && cbin < kD && r > 0 && r < h - 1 && c > 0 &&
          c < w - 1) {
        const double dx =
            (double)img[(int64_t)r * w + c + 1] - (double)img[(int64_t)r * w + c - 1];
        const double dy =
            (double)img[(int64_t)(r - 1) * w + c] - (double)img[(int64_t)(r + 1) * w + c];
        const double wgt = exp((c_rot * c_rot + r_rot * r_rot) * exp_scale);
        double a = atan2(dy, dx) * kDeg;
        if (a < 0.0) a += 360.0;
        double obin = (a - ori) * bins_per_deg;
        const double rf = floor(rbin), cf = floor(cbin), of = floor(obin);
        int o0 = (int)of;
        if (o0 < 0) o0 += kN;
        if (o0 >= kN) o0 -= kN;
        if (o0 >= 0 && o0 < kN) {  // always, for an angle in [0, 360)
          r0 = (int)rf;
          s_c0[lane] = (int)cf;
          s_o0[lane] = o0;
          s_mag[lane] = sqrt(dx * dx + dy * dy) * wgt;
          s_rb[lane] = rbin - rf;
          s_cb[lane] = cbin - cf;
          s_ob[lane] = obin - of;
        }
      }
    }
    s_r0[lane] = r0;
    __syncthreads();
    if (lane < (kD + 2) * (kD + 2)) {
      for (int t = 0; t < 64; ++t) {
        const int dr = R - s_r0[t], dc = C - s_c0[t];
        if (s_r0[t] == -2 || dr < 0 || dr > 1 || dc < 0 || dc > 1) continue;
        const double mag = s_mag[t], v_r1 = mag * s_rb[t];
        const double v_r = dr ? v_r1 : mag - v_r1;
        const double v_rc1 = v_r * s_cb[t];
        const double v_rc = dc ? v_rc1 : v_r - v_rc1;
        const double v1 = v_rc * s_ob[t];
        const int k = lane * (kN + 2) + s_o0[t];
        s_hist[k] += v_rc - v1;
        s_hist[k + 1] += v1;
      }
    }
    __syncthreads();
  }
  // the circular orientation bins, then normalise, clamp at 0.2, renormalise to 512, saturate:
  // the sums run in element order on one lane
#define H(p, q, k) s_hist[(((p) + 1) * (kD + 2) + (q) + 1) * (kN + 2) + (k)]
  if (lane == 0) {
    double nrm2 = 0.0;
    for (int p = 0; p < kD; ++p)
      for (int q = 0; q < kD; ++q) {
        H(p, q, 0) += H(p, q, kN);
        H(p, q, 1) += H(p, q, kN + 1);
        for (int k = 0; k < kN; ++k) nrm2 += H(p, q, k) * H(p, q, k);
      }
    const double thr = sqrt(nrm2) * 0.2;
    nrm2 = 0.0;
    for (int p = 0; p < kD; ++p)
      for (int q = 0; q < kD; ++q)
        for (int k = 0; k < kN; ++k) {
          const double v = H(p, q, k) < thr ? H(p, q, k) : thr;
          H(p, q, k) = v;
          nrm2 += v * v;
        }
    const double root = sqrt(nrm2);
    s_scale = 512.0 / (root > kFltEps ? root : kFltEps);
  }
  __syncthreads();
  for (int e = lane; e < kD * kD * kN; e += 64) {
    const double v = rint(H(e / (kD * kN), e / kN % kD, e % kN) * s_scale);
    dst[e] = (float)(v < 0.0 ? 0.0 : v > 255.0 ? 255.0 : v);
  }
#undef H
}

// ---- workspace of lgnn_sift_keypoints / lgnn_sift_gather ----------------------------------------

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct KeypointWs {
  Refined* ref;
  int32_t *npk, *koff, *kstart, *alive, *rank, *kept;
  float *angles, *thr;
  Keypoint* kp;
  size_t bytes;
};

KeypointWs keypoint_ws(void* base, int batch, int n) {
  KeypointWs ws;
  size_t at = 0;
  char* p = (char*)base;
  const size_t cap = (size_t)n * kMaxPeaks;
  auto take = [&](size_t bytes) {
    char* q = p + at;
    at += align256(bytes);
    return q;
  };
  ws.ref = (Refined*)take(sizeof(Refined) * n);
  ws.npk = (int32_t*)take(4 * (size_t)n);
  ws.koff = (int32_t*)take(4 * ((size_t)n + 1));
  ws.kstart = (int32_t*)take(4 * ((size_t)batch + 1));
  ws.kept = (int32_t*)take(4 * (size_t)batch);
  ws.thr = (float*)take(4 * (size_t)batch);
  ws.angles = (float*)take(4 * cap);
  ws.kp = (Keypoint*)take(sizeof(Keypoint) * cap);
  ws.alive = (int32_t*)take(4 * cap);
  ws.rank = (int32_t*)take(4 * cap);
  ws.bytes = at;
  return ws;
}

constexpr int kMaxCandidates = (1 << 26) / kMaxPeaks;  // the keypoint capacity stays far below 2^31

}  // namespace

// ---- entries ----------------------------------------------------------------------------------

extern "C" int lgnn_sift_num_octaves(int height, int width) {
  return dims_ok(1, height, width) ? octaves(1, height, width).n : 0;
}

extern "C" size_t lgnn_sift_pyramid_floats(int batch, int height, int width) {
  if (!dims_ok(batch, height, width)) return 0;
  const Octaves oc = octaves(batch, height, width);
  return (size_t)oc.goff[oc.n];
}

extern "C" int lgnn_sift_pyramid(const uint8_t* image, int batch, int height, int width,
                                 int channels, double sigma, uint8_t* gray, float* gauss,
                                 size_t gauss_floats, float* dog, size_t dog_floats,
                                 void* stream) {
  if (!dims_ok(batch, height, width) || (channels != 1 && channels != 3) || !sigma_ok(sigma))
    return LGNN_EINVAL;
  const Octaves oc = octaves(batch, height, width);
  if (!image || !gray || gauss_floats < (size_t)oc.goff[oc.n] ||
      dog_floats < (size_t)oc.doff[oc.n] || (oc.n && (!gauss || !dog)))
    return LGNN_EINVAL;
  hipStream_t st = as_stream(stream);
  const int64_t npix = (int64_t)batch * height * width;
  k_gray<<<(unsigned)((npix + 255) / 256), 256, 0, st>>>(image, npix, channels, gray);
  if (const int e = last_error()) return e;
  Taps taps[kLevels];
  make_taps(base_sigma(sigma), &taps[0]);
  for (int i = 1; i < kLevels; ++i) make_taps(level_sigma(sigma, i), &taps[i]);
  for (int o = 0; o < oc.n; ++o) {
    const int h = oc.h[o], w = oc.w[o];
    const int64_t plane = (int64_t)h * w;
    float* g = gauss + oc.goff[o];
    float* d = dog + oc.doff[o];
    const dim3 grid((w + kTile - 1) / kTile, (h + kTile - 1) / kTile, batch);
    if (o == 0) {
      k_blur<true><<<grid, 256, 0, st>>>(gray, (int64_t)height * width, g, kLevels * plane,
                                         nullptr, 0, h, w, taps[0]);
    } else {
      const int ph = oc.h[o - 1], pw = oc.w[o - 1];
      k_down<<<dim3((unsigned)((plane + 255) / 256), batch), 256, 0, st>>>(
          gauss + oc.goff[o - 1] + (int64_t)kLayers * ph * pw, (int64_t)kLevels * ph * pw, pw, g,
          kLevels * plane, h, w);
    }
    if (const int e = last_error()) return e;
    for (int i = 1; i < kLevels; ++i) {
      k_blur<false><<<grid, 256, 0, st>>>(g + (i - 1) * plane, kLevels * plane, g + i * plane,
                                          kLevels * plane, d + (i - 1) * plane, kDogs * plane, h,
                                          w, taps[i]);
      if (const int e = last_error()) return e;
    }
  }
  return LGNN_OK;
}

extern "C" size_t lgnn_sift_rows(int batch, int height, int width) {
  if (!dims_ok(batch, height, width)) return 0;
  const Octaves oc = octaves(batch, height, width);
  return (size_t)batch * oc.rowbase[oc.n];
}

extern "C" int lgnn_sift_count(const float* dog, int batch, int height, int width,
                               int32_t* counts, int32_t* row_ptr, void* stream) {
  if (!dims_ok(batch, height, width) || !counts || !row_ptr) return LGNN_EINVAL;
  const Octaves oc = octaves(batch, height, width);
  const int rows = batch * oc.rowbase[oc.n];
  if (rows && !dog) return LGNN_EINVAL;
  hipStream_t st = as_stream(stream);
  if (rows) {
    k_extrema<false><<<(rows + 3) / 4, 256, 0, st>>>(dog, oc, rows, counts, nullptr, nullptr, 0);
    if (const int e = last_error()) return e;
  }
  launch_exclusive_scan(counts, rows, row_ptr, st);
  return last_error();
}

extern "C" int lgnn_sift_candidates(const float* dog, int batch, int height, int width,
                                    const int32_t* row_ptr, int32_t* cand, int capacity,
                                    void* stream) {
  if (!dims_ok(batch, height, width) || !row_ptr || capacity < 0 || (capacity && !cand))
    return LGNN_EINVAL;
  const Octaves oc = octaves(batch, height, width);
  const int rows = batch * oc.rowbase[oc.n];
  if (!rows || !capacity) return LGNN_OK;
  if (!dog) return LGNN_EINVAL;
  k_extrema<true><<<(rows + 3) / 4, 256, 0, as_stream(stream)>>>(dog, oc, rows, nullptr, row_ptr,
                                                                cand, capacity);
  return last_error();
}

extern "C" size_t lgnn_sift_keypoints_workspace_bytes(int batch, int num_candidates) {
  if (batch < 1 || num_candidates < 0 || num_candidates > kMaxCandidates) return 0;
  return keypoint_ws(nullptr, batch, num_candidates > 0 ? num_candidates : 1).bytes;
}

extern "C" int lgnn_sift_keypoints(const float* gauss, const float* dog, int batch, int height,
                                   int width, double sigma, const int32_t* cand,
                                   int num_candidates, int num_keypoints, int64_t* node_ptr,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  if (!dims_ok(batch, height, width) || !sigma_ok(sigma) || num_keypoints < 1 ||
      num_candidates < 0 || num_candidates > kMaxCandidates || !node_ptr || !workspace)
    return LGNN_EINVAL;
  if (workspace_bytes < lgnn_sift_keypoints_workspace_bytes(batch, num_candidates) ||
      (num_candidates && (!gauss || !dog || !cand)))
    return LGNN_EINVAL;
  const Octaves oc = octaves(batch, height, width);
  hipStream_t st = as_stream(stream);
  const int n = num_candidates, cap = n * kMaxPeaks;
  const KeypointWs ws = keypoint_ws(workspace, batch, n > 0 ? n : 1);
  if (n) {
    k_refine<<<(n + 63) / 64, 64, 0, st>>>(dog, oc, batch, sigma, cand, n, ws.ref);
    if (const int e = last_error()) return e;
    k_orient<<<n, 64, 0, st>>>(gauss, oc, batch, cand, ws.ref, n, ws.npk, ws.angles);
    if (const int e = last_error()) return e;
  }
  launch_exclusive_scan(ws.npk, n, ws.koff, st);
  if (const int e = last_error()) return e;
  k_ranges<<<(batch + 256) / 256, 256, 0, st>>>(cand, n, ws.koff, batch, ws.kstart, ws.thr,
                                                ws.kept);
  if (const int e = last_error()) return e;
  if (n) {
    k_flatten<<<(n + 63) / 64, 64, 0, st>>>(cand, ws.ref, ws.npk, ws.koff, ws.angles, n, cap,
                                            ws.kp);
    if (const int e = last_error()) return e;
    const int blocks = (cap + 63) / 64;
    k_dedupe<<<blocks, 64, 0, st>>>(ws.kp, ws.kstart, batch, cap, ws.alive);
    if (const int e = last_error()) return e;
    k_rank<<<blocks, 64, 0, st>>>(ws.kp, ws.kstart, batch, cap, ws.alive, num_keypoints, ws.rank,
                                  ws.thr);
    if (const int e = last_error()) return e;
    k_keep<<<blocks, 64, 0, st>>>(ws.kp, ws.kstart, batch, cap, ws.alive, ws.thr, ws.kept);
    if (const int e = last_error()) return e;
  }
  launch_exclusive_scan(ws.kept, batch, node_ptr, st);
  return last_error();
}

extern "C" int lgnn_sift_gather(int batch, int num_candidates, const int64_t* node_ptr,
                                int total_nodes, float* kf, int32_t* ki, void* workspace,
                                size_t workspace_bytes, void* stream) {
  if (batch < 1 || num_candidates < 0 || num_candidates > kMaxCandidates || total_nodes < 0 ||
      !node_ptr || !workspace ||
      workspace_bytes < lgnn_sift_keypoints_workspace_bytes(batch, num_candidates))
    return LGNN_EINVAL;
  if (!total_nodes || !num_candidates) return LGNN_OK;
  if (!kf || !ki) return LGNN_EINVAL;
  const int cap = num_candidates * kMaxPeaks;
  const KeypointWs ws = keypoint_ws(workspace, batch, num_candidates);
  k_gather<<<(cap + 63) / 64, 64, 0, as_stream(stream)>>>(ws.kp, ws.kstart, batch, cap, ws.alive,
                                                         ws.rank, ws.thr, node_ptr, total_nodes,
                                                         kf, ki);
  return last_error();
}

extern "C" int lgnn_sift_descriptors(const float* gauss, int batch, int height, int width,
                                     const float* kf, const int32_t* ki, int num_nodes, float* x,
                                     void* stream) {
  if (!dims_ok(batch, height, width) || num_nodes < 0) return LGNN_EINVAL;
  if (!num_nodes) return LGNN_OK;
  if (!gauss || !kf || !ki || !x) return LGNN_EINVAL;
  const Octaves oc = octaves(batch, height, width);
  k_descriptors<<<num_nodes, 64, 0, as_stream(stream)>>>(gauss, oc, batch, kf, ki, num_nodes, x);
  return last_error();
}
