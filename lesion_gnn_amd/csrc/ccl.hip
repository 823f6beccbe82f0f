// Lesion nodes from a segmentation output: class map, connected components, component statistics.
// Reference: src/lesion_gnn/datasets/nodes/lesions.py:150-160 — torch.argmax +
// F.adaptive_max_pool2d on the GPU, .byte().cpu().numpy(), then
// cv2.connectedComponentsWithStatsWithAlgorithm(connectivity=8) on the host and the labels copied
// back. Here the chain stays on the device.
//
// k_label_pool  — one thread per output pixel: the argmax over the classes of every input pixel
//                 of its pooling window (first index among equal maxima), the largest of them.
// Labelling (lgnn_ccl) is a union-find over an int32 parent word per pixel (background -1), in
// which a parent is never larger than its child: the root of a component is its first pixel in
// raster order, so ranking the roots numbers the components as the contract asks.
// k_ccl_init    — a wave takes 64 consecutive pixels of a row: one ballot gives every lane the
//                 start of its run inside the segment, which becomes its parent. No atomics.
// k_ccl_merge   — the links the init left out: a run continuing across a segment border, and the
//                 row above (N, or NW / NE where N is background; a pixel whose left neighbour is
//                 foreground leaves to it what that neighbour already links). Unions by atomicMin
//                 on the larger root, retried with the value the atomic returned; every parent
//                 word is read with an agent-scope atomic load (another workgroup, possibly on
//                 another XCD, may be changing it).
// k_ccl_compress— every pixel's parent becomes its root; roots counted per 1024-pixel block.
// k_ccl_scan    — one workgroup: exclusive scan of the block counts, num_labels.
// k_ccl_rank    — root -> 1 + its rank among the roots.
// k_ccl_label   — labels[p] = rank of the root of p.
// The phases are separate launches: no workgroup waits on another inside one.
// Statistics (lgnn_ccl_stats): integer min / max / count / coordinate sums per label. A lane walks
// 8 consecutive pixels and keeps one (label, partial) run in registers; a run goes to the
// workgroup's LDS bins (labels below 1024: the background, which holds most pixels of a lesion
// map, is label 0) or, above, to global memory; the touched bins leave as one global integer
// atomic each. Integer sums: any order gives the same bits.
// Every kernel carries an image dimension (ccl.h; the batch entries are in ccl_batch.hip): B
// images of one size are labelled as one image of B * H rows in which the merge links nothing
// across a multiple of H; roots are counted and ranked in per-image blocks, so the numbering
// restarts with each image and the scan's offsets at the images' first blocks are node_ptr.
#include <algorithm>
#include <climits>

#include "ccl.h"
#include "wg.h"

namespace lgnn_cclk {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSeg = 64;        // pixels of one row per wave (init, merge)
constexpr int kScanPix = 1024;  // pixels per workgroup (compress, rank): 4 per thread
constexpr int kScanThreads = 1024;
constexpr int kBins = 1024;     // labels with LDS bins (stats)
constexpr int kRun = 8;         // consecutive pixels per lane (stats)

__global__ void __launch_bounds__(kThreads)
    k_label_pool(const float* __restrict__ logits, int B, int K, int Hin, int Win,
                 uint8_t* __restrict__ out, int H, int W) {
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= (int64_t)B * H * W) return;
  const int64_t b = g / ((int64_t)H * W), o = g - b * H * W;
  const int oy = (int)(o / W), ox = (int)(o - (int64_t)oy * W);
  const int y0 = (int)((int64_t)oy * Hin / H), y1 = (int)(((int64_t)(oy + 1) * Hin + H - 1) / H);
  const int x0 = (int)((int64_t)ox * Win / W), x1 = (int)(((int64_t)(ox + 1) * Win + W - 1) / W);
  const int64_t plane = (int64_t)Hin * Win;
  logits += b * K * plane;
  int best = 0;
  for (int y = y0; y < y1; ++y)
    for (int x = x0; x < x1; ++x) {
      const float* q = logits + (int64_t)y * Win + x;
      float m = q[0];
      int a = 0;
      for (int k = 1; k < K; ++k) {
        const float v = q[k * plane];
        if (v > m || (v != v && m == m)) {  // torch.argmax: a NaN is the maximum, the first wins
          m = v;
          a = k;
        }
      }
      best = max(best, a);
    }
  out[g] = (uint8_t)best;
}

__device__ __forceinline__ int32_t ld_agent(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// parent[x] <= x for every x at all times, so the walk strictly descends until a fixed point.
// A value read late is still an ancestor of x: parents are only ever replaced by smaller members
// of the same component.
__device__ __forceinline__ int32_t find_root(const int32_t* parent, int32_t x) {
  int32_t p = ld_agent(parent + x);
  while (p != x) {
    x = p;
    p = ld_agent(parent + x);
  }
  return x;
}

// The same walk in the merge launch, where it also points every node it passes at its grandparent
// (an ancestor, and smaller: still a decrease), so that the links of a long run's segments, made
// one by one, do not grow into a chain every later walk follows to its end.
__device__ __forceinline__ int32_t find_root_split(int32_t* parent, int32_t x) {
  int32_t p = ld_agent(parent + x);
  while (p != x) {
    const int32_t g = ld_agent(parent + p);
    if (g != p) atomicMin(parent + x, g);
    x = p;
    p = g;
  }
  return x;
}

// Link the components of a and b. The atomicMin either finds the larger root still a root (done)
// or returns the smaller parent another lane gave it; the retry starts from that value. max(a, b)
// strictly decreases from one iteration to the next, so the loop ends.
__device__ __forceinline__ void unite(int32_t* parent, int32_t a, int32_t b) {
  for (;;) {
    a = find_root_split(parent, a);
    b = find_root_split(parent, b);
    if (a == b) return;
    if (a < b) {
      const int32_t t = a;
      a = b;
      b = t;
    }
    const int32_t old = atomicMin(parent + a, b);
    if (old == a) return;
    a = old;
  }
}

// wave -> (row y, 64-pixel segment of it); false past the image (wave-uniform)
__device__ __forceinline__ bool seg_task(int H, int nseg, int& y, int& x0) {
  const int64_t task = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (task >= (int64_t)H * nseg) return false;
  y = (int)(task / nseg);
  x0 = (int)(task - (int64_t)y * nseg) * kSeg;
  return true;
}

__global__ void __launch_bounds__(kThreads)
    k_ccl_init(const uint8_t* __restrict__ img, int H, int W, int nseg,
               int32_t* __restrict__ parent) {
  int y, x0;
  if (!seg_task(H, nseg, y, x0)) return;
  const int lane = threadIdx.x & 63, x = x0 + lane;
  const bool fg = x < W && img[(int64_t)y * W + x] != 0;
  const unsigned long long mask = __ballot(fg);
  if (x >= W) return;
  // the run of lane starts one past the highest background lane below it
  const unsigned long long below = ~mask & ((1ull << lane) - 1ull);
  const int start = below ? 64 - __clzll(below) : 0;
  parent[y * W + x] = fg ? y * W + x0 + start : -1;
}

template <bool k8>
__global__ void __launch_bounds__(kThreads)
    k_ccl_merge(const uint8_t* __restrict__ img, int rows, int H, int W, int nseg,
                int32_t* parent) {
  int y, x0;
  if (!seg_task(rows, nseg, y, x0)) return;
  const int lane = threadIdx.x & 63, x = x0 + lane;
  const bool fg = x < W && img[(int64_t)y * W + x] != 0;
  const unsigned long long mask = __ballot(fg);
  if (!fg) return;
  const int p = y * W + x;
  bool left;
  if (lane > 0) {
    left = (mask >> (lane - 1)) & 1ull;
  } else {
    left = x > 0 && img[(int64_t)p - 1] != 0;
    if (left) unite(parent, p, p - 1);  // the run continues across the segment border
  }
  if (y % H == 0) return;  // the first row of an image: nothing above it belongs to it
  const uint8_t* up = img + (int64_t)(y - 1) * W;
  const bool n = up[x] != 0;
  // By induction along a row's run, a pixel ends up linked to every foreground pixel among its
  // W, NW, N, NE (8) or W, N (4): the run's first pixel links them itself (through N where N is
  // foreground: NW and NE touch N in the row above); a later pixel gets NW and N through its left
  // neighbour, whose N and NE they are, and links NE itself only where N does not carry it.
  if (k8) {
    const bool ne = x + 1 < W && up[x + 1] != 0;
    if (left) {
      if (!n && ne) unite(parent, p, p - W + 1);
    } else if (n) {
      unite(parent, p, p - W);
    } else {
      if (x > 0 && up[x - 1] != 0) unite(parent, p, p - W - 1);
      if (ne) unite(parent, p, p - W + 1);
    }
  } else {
    // 4: N is reached through the left neighbour when that one's own N is foreground too
    if (n && !(left && up[x - 1] != 0)) unite(parent, p, p - W);
  }
}

__global__ void __launch_bounds__(kThreads)
    k_ccl_compress(int32_t* parent, int64_t hw, int nbi, int32_t* __restrict__ blockcount) {
  __shared__ int32_t wsum[kWaves];
  // nbi blocks per image: no block holds roots of two images
  const int b = blockIdx.x / nbi;
  const int64_t local = (int64_t)(blockIdx.x - b * nbi) * kScanPix + threadIdx.x * 4;
  int c = 0;
  for (int j = 0; j < 4; ++j) {
    if (local + j >= hw) break;
    const int64_t p = b * hw + local + j;
    const int32_t q = ld_agent(parent + p);
    if (q < 0) continue;
    const int32_t r = find_root(parent, q);
    // roots are final since the merge launch ended; a concurrent walk through p reads the old
    // parent or the root, both ancestors
    if (r != q) __hip_atomic_store(parent + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    c += r == (int32_t)p;
  }
  const int s = block_sum<kThreads>(c, wsum);
  if (threadIdx.x == 0) blockcount[blockIdx.x] = s;
}

__global__ void __launch_bounds__(kScanThreads)
    k_ccl_scan(int32_t* blockcount, int nb, int nbi, int B, int32_t* __restrict__ num_labels,
               int64_t* __restrict__ node_ptr) {
  __shared__ int32_t wsum[kScanThreads / 64];
  int carry = 0;
  for (int base = 0; base < nb; base += kScanThreads) {
    const int i = base + threadIdx.x;
    const int at = block_exclusive_scan<kScanThreads>(i < nb ? blockcount[i] : 0, carry, wsum);
    if (i < nb) blockcount[i] = at;
  }
  __syncthreads();  // the offsets below were written by other threads
  // per image: its roots are the difference of the offsets of its first block and the next image's
  for (int b = threadIdx.x; b < B; b += kScanThreads) {
    const int first = blockcount[b * nbi];
    const int next = b + 1 < B ? blockcount[(b + 1) * nbi] : carry;
    num_labels[b] = next - first + 1;
    if (node_ptr) node_ptr[b] = (int64_t)first + b;
  }
  if (threadIdx.x == 0 && node_ptr) node_ptr[B] = (int64_t)carry + B;
}

__global__ void __launch_bounds__(kThreads)
    k_ccl_rank(const int32_t* __restrict__ parent, int64_t hw, int nbi,
               const int32_t* __restrict__ blockoff, int32_t* __restrict__ rootlabel) {
  __shared__ int32_t wsum[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x / nbi;
  const int64_t local = (int64_t)(blockIdx.x - b * nbi) * kScanPix + threadIdx.x * 4;
  const int64_t base = b * hw + local;
  bool root[4];
  int c = 0;
  for (int j = 0; j < 4; ++j) {
    const int64_t p = base + j;
    root[j] = local + j < hw && parent[p] == (int32_t)p;
    c += root[j];
  }
  const int s = wave_inclusive_scan(c);
  if (lane == 63) wsum[wave] = s;
  __syncthreads();
  int r = blockoff[blockIdx.x] - blockoff[b * nbi] + s - c + 1;  // the rank restarts per image
  for (int w = 0; w < wave; ++w) r += wsum[w];
  for (int j = 0; j < 4; ++j)
    if (root[j]) rootlabel[base + j] = r++;
}

__global__ void __launch_bounds__(kThreads)
    k_ccl_label(const int32_t* __restrict__ parent, const int32_t* __restrict__ rootlabel,
                int64_t npix, int64_t* __restrict__ labels) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= npix) return;
  const int32_t q = parent[p];
  labels[p] = q < 0 ? 0 : rootlabel[q];
}

// ---- statistics ------------------------------------------------------------------------------

__global__ void __launch_bounds__(kThreads)
    k_stats_init(int n, int32_t* __restrict__ stats, unsigned long long* __restrict__ sums,
                 int32_t* __restrict__ err) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i == 0) *err = 0;
  if (i >= n) return;
  int32_t* s = stats + (int64_t)i * 5;
  s[0] = INT_MAX;  // min x
  s[1] = INT_MAX;  // min y
  s[2] = -1;       // max x, the width once finished
  s[3] = -1;       // max y, the height once finished
  s[4] = 0;
  sums[2 * (int64_t)i] = 0ull;
  sums[2 * (int64_t)i + 1] = 0ull;
}

__global__ void __launch_bounds__(kThreads)
    k_stats_acc(const int64_t* __restrict__ labels, int64_t npix, int W, int n, int chunks,
                int gpi, const int64_t* __restrict__ node_ptr, int32_t* __restrict__ stats,
                unsigned long long* __restrict__ sums, int32_t* __restrict__ err) {
  __shared__ int32_t b_minx[kBins], b_miny[kBins], b_maxx[kBins], b_maxy[kBins], b_area[kBins];
  __shared__ unsigned long long b_sx[kBins], b_sy[kBins];
  // gpi workgroups per image of npix pixels. With node_ptr (a batch) image b's labels own the
  // rows [node_ptr[b], node_ptr[b + 1]) of the n rows; offsets that leave them own none.
  const int img = blockIdx.x / gpi, blk = blockIdx.x - img * gpi;
  labels += (int64_t)img * npix;
  if (node_ptr) {
    const int64_t r0 = node_ptr[img], r1 = node_ptr[img + 1];
    const bool ok = r0 >= 0 && r0 <= r1 && r1 <= n;
    n = ok ? (int)(r1 - r0) : 0;
    stats += (ok ? r0 : 0) * 5;
    sums += (ok ? r0 : 0) * 2;
  }
  const int nb = min(n, kBins);
  for (int i = threadIdx.x; i < nb; i += kThreads) {
    b_minx[i] = INT_MAX;
    b_miny[i] = INT_MAX;
    b_maxx[i] = -1;
    b_maxy[i] = -1;
    b_area[i] = 0;
    b_sx[i] = 0ull;
    b_sy[i] = 0ull;
  }
  __syncthreads();

  int bad = 0;
  for (int c = 0; c < chunks; ++c) {
    const int64_t p0 =
        ((int64_t)blk * chunks + c) * (kThreads * kRun) + (int64_t)threadIdx.x * kRun;
    if (p0 >= npix) break;
    int y = (int)(p0 / W), x = (int)(p0 - (int64_t)y * W);
    int cur = -1, minx = 0, maxx = 0, miny = 0, maxy = 0, area = 0;
    unsigned long long sx = 0ull, sy = 0ull;
    auto flush = [&]() {
      if (cur < 0) return;
      if (cur < nb) {
        atomicMin(&b_minx[cur], minx);
        atomicMin(&b_miny[cur], miny);
        atomicMax(&b_maxx[cur], maxx);
        atomicMax(&b_maxy[cur], maxy);
        atomicAdd(&b_area[cur], area);
        atomicAdd(&b_sx[cur], sx);
        atomicAdd(&b_sy[cur], sy);
      } else {
        int32_t* s = stats + (int64_t)cur * 5;
        atomicMin(s + 0, minx);
        atomicMin(s + 1, miny);
        atomicMax(s + 2, maxx);
        atomicMax(s + 3, maxy);
        atomicAdd(s + 4, area);
        atomicAdd(sums + 2 * (int64_t)cur, sx);
        atomicAdd(sums + 2 * (int64_t)cur + 1, sy);
      }
    };
    const int m = (int)min((int64_t)kRun, npix - p0);
    for (int j = 0; j < m; ++j) {
      const int64_t l = labels[p0 + j];
      if (l < 0 || l >= n) {
        ++bad;
      } else if ((int)l != cur) {
        flush();
        cur = (int)l;
        minx = maxx = x;
        miny = maxy = y;
        area = 1;
        sx = (unsigned long long)x;
        sy = (unsigned long long)y;
      } else {
        minx = min(minx, x);
        maxx = max(maxx, x);
        maxy = y;  // rows only grow along a lane's pixels
        ++area;
        sx += (unsigned long long)x;
        sy += (unsigned long long)y;
      }
      if (++x == W) {
        x = 0;
        ++y;
      }
    }
    flush();
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nb; i += kThreads) {
    if (!b_area[i]) continue;
    int32_t* s = stats + (int64_t)i * 5;
    atomicMin(s + 0, b_minx[i]);
    atomicMin(s + 1, b_miny[i]);
    atomicMax(s + 2, b_maxx[i]);
    atomicMax(s + 3, b_maxy[i]);
    atomicAdd(s + 4, b_area[i]);
    atomicAdd(sums + 2 * (int64_t)i, b_sx[i]);
    atomicAdd(sums + 2 * (int64_t)i + 1, b_sy[i]);
  }
  bad = wave_sum(bad);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(err, bad);
}

// the integer sums sit in the centroid words; each label's thread reads both before it writes
__global__ void __launch_bounds__(kThreads)
    k_stats_finish(int n, int32_t* __restrict__ stats, double* centroids) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  int32_t* s = stats + (int64_t)i * 5;
  const unsigned long long* sums = reinterpret_cast<const unsigned long long*>(centroids);
  const unsigned long long sx = sums[2 * (int64_t)i], sy = sums[2 * (int64_t)i + 1];
  const int area = s[4];
  if (area == 0) {
    s[0] = s[1] = s[2] = s[3] = 0;
    centroids[2 * (int64_t)i] = 0.0;
    centroids[2 * (int64_t)i + 1] = 0.0;
    return;
  }
  s[2] = s[2] - s[0] + 1;
  s[3] = s[3] - s[1] + 1;
  centroids[2 * (int64_t)i] = (double)(long long)sx / (double)area;
  centroids[2 * (int64_t)i + 1] = (double)(long long)sy / (double)area;
}

// ---- launches: one image (lgnn_label_pool, lgnn_ccl, lgnn_ccl_stats below) or a batch of equal
// ---- size (ccl_batch.hip); arguments are checked by the entries -------------------------------

bool image_dims_ok(int H, int W) {
  return H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31);
}
bool batch_dims_ok(int B, int H, int W) {
  return B > 0 && image_dims_ok(H, W) && (int64_t)B * H * W < ((int64_t)1 << 31);
}
static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

int launch_label_pool(const float* logits, int B, int K, int Hin, int Win, uint8_t* out, int H,
                      int W, hipStream_t s) {
  const int64_t npix = (int64_t)B * H * W;
  return launch(k_label_pool, dim3((unsigned)((npix + kThreads - 1) / kThreads)), dim3(kThreads), s,
                logits, B, K, Hin, Win, out, H, W);
}

size_t ccl_workspace_bytes(int B, int H, int W) {
  const int64_t hw = (int64_t)H * W;
  const int64_t nb = B * ((hw + kScanPix - 1) / kScanPix);
  return 2 * align256((size_t)(B * hw) * sizeof(int32_t)) + align256((size_t)nb * sizeof(int32_t));
}

// The batch is one image of B * H rows in which no link crosses a multiple of H, its roots
// counted and ranked in blocks that end with each image. num_labels [B]; node_ptr [B + 1] or NULL.
int launch_ccl(const uint8_t* image, int B, int H, int W, int connectivity, int64_t* labels,
               int32_t* num_labels, int64_t* node_ptr, void* workspace, hipStream_t s) {
  const int64_t hw = (int64_t)H * W, npix = B * hw;
  const int rows = B * H;
  const int nbi = (int)((hw + kScanPix - 1) / kScanPix), nb = B * nbi;
  char* ws = static_cast<char*>(workspace);
  int32_t* parent = reinterpret_cast<int32_t*>(ws);
  ws += align256((size_t)npix * sizeof(int32_t));
  int32_t* rootlabel = reinterpret_cast<int32_t*>(ws);
  ws += align256((size_t)npix * sizeof(int32_t));
  int32_t* blockcount = reinterpret_cast<int32_t*>(ws);

  const int nseg = (W + kSeg - 1) / kSeg;
  const dim3 sgrid((unsigned)(((int64_t)rows * nseg + kWaves - 1) / kWaves));
  if (const int e = launch(k_ccl_init, sgrid, dim3(kThreads), s, image, rows, W, nseg,
                           parent)) return e;
  one_of<false, true>(connectivity == 8, [&](auto DIAG) {
    enqueue(k_ccl_merge<DIAG>, sgrid, dim3(kThreads), s, image, rows, H, W, nseg, parent);
  });
  if (const int e = last_error()) return e;
  if (const int e = launch(k_ccl_compress, dim3(nb), dim3(kThreads), s, parent, hw, nbi,
                           blockcount)) return e;
  if (const int e = launch(k_ccl_scan, dim3(1), dim3(kScanThreads), s, blockcount, nb, nbi, B,
                           num_labels, node_ptr)) return e;
  if (const int e = launch(k_ccl_rank, dim3(nb), dim3(kThreads), s, parent, hw, nbi, blockcount,
                           rootlabel)) return e;
  return launch(k_ccl_label, dim3((unsigned)((npix + kThreads - 1) / kThreads)), dim3(kThreads), s,
                parent, rootlabel, npix, labels);
}

// labels [B, H, W] -> num_rows rows of stats and centroids: the rows of image b start at
// node_ptr[b] (device), or at 0 for the one image of node_ptr == NULL.
int launch_ccl_stats(const int64_t* labels, int B, int H, int W, const int64_t* node_ptr,
                     int num_rows, int32_t* stats, double* centroids, int32_t* err,
                     hipStream_t s) {
  const int64_t hw = (int64_t)H * W;
  unsigned long long* sums = reinterpret_cast<unsigned long long*>(centroids);
  const dim3 lgrid((unsigned)((num_rows + kThreads - 1) / kThreads));
  if (const int e = launch(k_stats_init, lgrid, dim3(kThreads), s, num_rows, stats, sums,
                           err)) return e;
  const int64_t chunk = (int64_t)kThreads * kRun;
  const int64_t nchunks = (hw + chunk - 1) / chunk;
  const int gpi = (int)std::min<int64_t>(nchunks, 1024);
  const int chunks = (int)((nchunks + gpi - 1) / gpi);
  if (const int e = launch(k_stats_acc, dim3((unsigned)((int64_t)B * gpi)), dim3(kThreads), s,
                           labels, hw, W, num_rows, chunks, gpi, node_ptr, stats, sums,
                           err)) return e;
  return launch(k_stats_finish, lgrid, dim3(kThreads), s, num_rows, stats, centroids);
}

}  // namespace lgnn_cclk

using namespace lgnn_cclk;

extern "C" int lgnn_label_pool(const float* logits, int classes, int in_height, int in_width,
                               uint8_t* out, int height, int width, void* stream) {
  if (classes < 1 || classes > 255 || !image_dims_ok(in_height, in_width) ||
      !image_dims_ok(height, width) || !logits || !out)
    return LGNN_EINVAL;
  return launch_label_pool(logits, 1, classes, in_height, in_width, out, height, width,
                           as_stream(stream));
}

extern "C" size_t lgnn_ccl_workspace_bytes(int height, int width) {
  return image_dims_ok(height, width) ? ccl_workspace_bytes(1, height, width) : 0;
}

extern "C" int lgnn_ccl(const uint8_t* image, int height, int width, int connectivity,
                        int64_t* labels, int32_t* num_labels, void* workspace,
                        size_t workspace_bytes, void* stream) {
  if ((connectivity != 4 && connectivity != 8) || !image_dims_ok(height, width)) return LGNN_EINVAL;
  if (!image || !labels || !num_labels || !workspace ||
      workspace_bytes < lgnn_ccl_workspace_bytes(height, width))
    return LGNN_EINVAL;
  return launch_ccl(image, 1, height, width, connectivity, labels, num_labels, nullptr, workspace,
                    as_stream(stream));
}

extern "C" int lgnn_ccl_stats(const int64_t* labels, int height, int width, int num_labels,
                              int32_t* stats, double* centroids, int32_t* err, void* stream) {
  if (!image_dims_ok(height, width) || num_labels < 1) return LGNN_EINVAL;
  if (!labels || !stats || !centroids || !err) return LGNN_EINVAL;
  return launch_ccl_stats(labels, 1, height, width, nullptr, num_labels, stats, centroids, err,
                          as_stream(stream));
}

