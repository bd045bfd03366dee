// Connected-component labelling: the mask refinement behind the background remover (reference
// actionmesh/preprocessing/background_removal.py:20-38: Otsu threshold, skimage.measure.label, remove_small_objects) and the
// component search of the floater removal (actionmesh/preprocessing/mesh_processor.py:288-325: trimesh's mesh.split).  The contract
// is include/actionmesh_amd.h's; both results are fully determined (a label is the smallest index of its component), so they are
// compared bit for bit with scipy.
//
//   One union-find for both: L[i] is the parent of element i, a root has L[i] == i, and a parent is ALWAYS SMALLER than its child.
//   So there is no cycle, the root of a finished component is its smallest element, and every write only ever lowers a word:
//     find   follows parents to the root (no write);
//     union  links the larger root under the smaller one with atomicMin and looks at what the word held before: if that was the
//            root itself the link stands, otherwise another thread re-parented it first and the union goes on from the parent it
//            saw (the link that atomicMin may have replaced is re-made by that very continuation).  A lock-free retry: no thread
//            waits for another, and it ends because labels only decrease.
//   Parents are read with agent-scope atomic loads, so a find inside the launch that also unions never walks a stale L1 line; the
//   verdict of a union is the atomic's own return value.  Kernels hand over to each other at launch boundaries only: no grid-wide
//   barrier, no flag, no spinning.  Integer atomics only (min on labels, add on sizes and counters): no result depends on scheduling.
//
//   am_mask_refine, whatever n_frames is (7 launches with Otsu, 5 with a fixed threshold):
//     zero        the histograms                                                         (Otsu only)
//     histogram   256 bins per frame: per-wave LDS histograms, then one global add per non-empty bin and workgroup   (Otsu only)
//     otsu        one wave per frame, one lane walks the 256 bins in fp64 (no contraction: the file is built with -ffp-contract=off)
//     tile        32 x 32 pixels per workgroup: threshold, union the W / NW / N / NE neighbours in LDS, write every pixel's
//                 tile-local root as a frame index (raster order inside a tile agrees with raster order in the frame)
//     merge       one thread per pixel of a tile's first column / first row: unions across the border, corners included
//     flatten     every pixel -> its root; component sizes by one add per (wave, root) - a giant component costs a wave one add
//     output      out_mask / out_labels / out_stats
//   am_graph_components: init, union over the edge list (validating it), flatten + sizes, size gather - the same device functions.
#include "am_common.h"

#include <float.h>

namespace {

constexpr int CC_TILE = 32;
constexpr int CC_THREADS = 256;
constexpr int CC_PPT = CC_TILE * CC_TILE / CC_THREADS;
constexpr int CC_HIST_CHUNK = 16;         // consecutive pixels one thread histograms at a time
constexpr int CC_HIST_MAX_BLOCKS = 64;    // per frame

__device__ __forceinline__ int uf_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void uf_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int uf_find(const int* L, int a) {
  for (int p; (p = uf_load(L + a)) != a;) a = p;
  return a;
}

__device__ __forceinline__ void uf_union(int* L, int a, int b) {
  for (;;) {
    a = uf_find(L, a);
    b = uf_find(L, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(L + a, b);        // a > b: a's word becomes min(what it held, b)
    if (old == a) return;                       // a was a root: linked
    a = old;                                    // a had parent `old` already: unite that parent with b
  }
}

// One add per distinct root among the wave's lanes (root < 0: the lane has nothing to count).  Wave-uniform control flow.
__device__ __forceinline__ void wave_count_roots(int* size, int root) {
  const int lane = threadIdx.x & 63;
  unsigned long long active = __ballot(root >= 0);
  while (active) {
    const int leader = __ffsll((long long)active) - 1;
    const int lr = __shfl(root, leader);
    const unsigned long long same = __ballot(root == lr);
    if (lane == leader) atomicAdd(size + lr, (int)__popcll(same));
    active &= ~same;
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_zero_kernel(uint32_t* __restrict__ p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (i < n) p[i] = 0u;
}

// grid (blocks per frame, n_frames)
__global__ __launch_bounds__(CC_THREADS) void cc_hist_kernel(const uint8_t* __restrict__ mask, int64_t hw, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[CC_THREADS / 64][256];
  const int t = threadIdx.x, wave = t >> 6;
  for (int w = 0; w < CC_THREADS / 64; ++w) h[w][t] = 0u;
  __syncthreads();
  const uint8_t* __restrict__ src = mask + (int64_t)blockIdx.y * hw;
  const int64_t stride = (int64_t)gridDim.x * CC_THREADS * CC_HIST_CHUNK;
  for (int64_t i0 = ((int64_t)blockIdx.x * CC_THREADS + t) * CC_HIST_CHUNK; i0 < hw; i0 += stride) {
    uint8_t px[CC_HIST_CHUNK];
    if (i0 + CC_HIST_CHUNK <= hw) {
      __builtin_memcpy(px, src + i0, CC_HIST_CHUNK);
    } else {
#pragma unroll
      for (int e = 0; e < CC_HIST_CHUNK; ++e) px[e] = i0 + e < hw ? src[i0 + e] : (uint8_t)0;
    }
    const int n = i0 + CC_HIST_CHUNK <= hw ? CC_HIST_CHUNK : (int)(hw - i0);
    // runs of equal values (a soft mask is mostly 0 and 255) cost one LDS atomic each
    int run = 1;
    uint8_t last = px[0];
#pragma unroll
    for (int e = 1; e < CC_HIST_CHUNK; ++e) {
      if (e >= n) continue;
      if (px[e] == last) {
        ++run;
      } else {
        atomicAdd(&h[wave][last], (uint32_t)run);
        last = px[e];
        run = 1;
      }
    }
    atomicAdd(&h[wave][last], (uint32_t)run);
  }
  __syncthreads();
  uint32_t s = 0;
  for (int w = 0; w < CC_THREADS / 64; ++w) s += h[w][t];
  if (s) atomicAdd(hist + (int64_t)blockIdx.y * 256 + t, s);
}

// grid n_frames, one wave.  OpenCV's getThreshVal_Otsu_8u restated (the header spells the loop): fp64, every operation rounded on its own.
__global__ __launch_bounds__(64) void cc_otsu_kernel(const uint32_t* __restrict__ hist, int64_t hw, int fixed, int32_t* __restrict__ thr,
                                                     int32_t* __restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ uint32_t h[256];
  const int f = blockIdx.x, lane = threadIdx.x;
  if (fixed < 0) {
    for (int i = lane; i < 256; i += 64) h[i] = hist[(int64_t)f * 256 + i];
  }
  __syncthreads();
  if (lane != 0) return;
  int max_val = fixed;
  if (fixed < 0) {
    const double scale = 1.0 / (double)hw;
    unsigned long long isum = 0;              // exact: below 255 * 2^31
    for (int i = 0; i < 256; ++i) isum += (unsigned long long)i * h[i];
    const double mu = (double)isum * scale;
    double mu1 = 0.0, q1 = 0.0, max_sigma = 0.0;
    max_val = 0;
    const double eps = (double)FLT_EPSILON, one_minus_eps = 1.0 - (double)FLT_EPSILON;
    for (int i = 0; i < 256; ++i) {
      const double p = (double)h[i] * scale;
      mu1 = mu1 * q1;
      q1 = q1 + p;
      const double q2 = 1.0 - q1;
      const double lo = q1 < q2 ? q1 : q2, hi = q1 < q2 ? q2 : q1;
      if (lo < eps || hi > one_minus_eps) continue;
      const double ip = (double)i * p;
      mu1 = (mu1 + ip) / q1;
      const double q1mu1 = q1 * mu1;
      const double mu2 = (mu - q1mu1) / q2;
      const double d = mu1 - mu2;
      const double q1q2 = q1 * q2;
      const double q1q2d = q1q2 * d;
      const double sigma = q1q2d * d;
      if (sigma > max_sigma) {
        max_sigma = sigma;
        max_val = i;
      }
    }
  }
  thr[f] = max_val;
  if (stats) {
    stats[f * 4 + 0] = max_val;
    stats[f * 4 + 1] = 0;
    stats[f * 4 + 2] = 0;
    stats[f * 4 + 3] = 0;
  }
}

// grid tiles_x * tiles_y * n_frames.  L: frame index of the pixel's tile-local root, -1 on background.  Also zeroes the sizes.
__global__ __launch_bounds__(CC_THREADS) void cc_tile_kernel(const uint8_t* __restrict__ mask, int height, int width, int tiles_x,
                                                             int tiles_per_frame, const int32_t* __restrict__ thr,
                                                             int* __restrict__ labels, int* __restrict__ sizes) {
  __shared__ int lab[CC_TILE * CC_TILE];
  const int t = threadIdx.x;
  const int f = blockIdx.x / tiles_per_frame, tile = blockIdx.x % tiles_per_frame;
  const int x0 = (tile % tiles_x) * CC_TILE, y0 = (tile / tiles_x) * CC_TILE;
  const int64_t base = (int64_t)f * height * width;
  const int th = thr[f];
#pragma unroll
  for (int k = 0; k < CC_PPT; ++k) {
    const int i = t + k * CC_THREADS, x = x0 + (i & (CC_TILE - 1)), y = y0 + (i >> 5);
    const bool fg = x < width && y < height && (int)mask[base + (int64_t)y * width + x] > th;
    lab[i] = fg ? i : -1;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CC_PPT; ++k) {
    const int i = t + k * CC_THREADS, lx = i & (CC_TILE - 1), ly = i >> 5;
    if (lab[i] < 0) continue;                   // the sign of a word never changes
    if (lx > 0 && lab[i - 1] >= 0) uf_union(lab, i, i - 1);
    if (ly > 0) {
      if (lab[i - CC_TILE] >= 0) uf_union(lab, i, i - CC_TILE);
      if (lx > 0 && lab[i - CC_TILE - 1] >= 0) uf_union(lab, i, i - CC_TILE - 1);
      if (lx < CC_TILE - 1 && lab[i - CC_TILE + 1] >= 0) uf_union(lab, i, i - CC_TILE + 1);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CC_PPT; ++k) {
    const int i = t + k * CC_THREADS, x = x0 + (i & (CC_TILE - 1)), y = y0 + (i >> 5);
    if (x >= width || y >= height) continue;
    int r = -1;
    if (lab[i] >= 0) {
      const int lr = uf_find(lab, i);
      r = (y0 + (lr >> 5)) * width + x0 + (lr & (CC_TILE - 1));
    }
    const int64_t p = base + (int64_t)y * width + x;
    labels[p] = r;
    sizes[p] = 0;
  }
}

// grid border_blocks * n_frames.  Border pixel k of a frame: the first column of every tile column but the first (height pixels each),
// then the first row of every tile row but the first (width pixels each).  A pair of 8-neighbours in different tiles has one pixel in
// a first column with the other at its W / NW / SW, or one in a first row with the other at its N / NW / NE.
__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(int* __restrict__ labels, int height, int width, int tiles_x, int border,
                                                              int border_blocks) {
  const int f = blockIdx.x / border_blocks;
  const int k = (blockIdx.x % border_blocks) * CC_THREADS + threadIdx.x;
  if (k >= border) return;
  int* L = labels + (int64_t)f * height * width;
  const int ncol = (tiles_x - 1) * height;
  int x, y;
  bool column;
  if (k < ncol) {
    x = (k / height + 1) * CC_TILE;
    y = k % height;
    column = true;
  } else {
    x = (k - ncol) % width;
    y = ((k - ncol) / width + 1) * CC_TILE;
    column = false;
  }
  const int p = y * width + x;
  if (L[p] < 0) return;
  int qx[3], qy[3];
  for (int j = 0; j < 3; ++j) {
    qx[j] = column ? x - 1 : x - 1 + j;
    qy[j] = column ? y - 1 + j : y - 1;
  }
  for (int j = 0; j < 3; ++j) {
    if (qx[j] < 0 || qx[j] >= width || qy[j] < 0 || qy[j] >= height) continue;
    const int q = qy[j] * width + qx[j];
    if (L[q] >= 0) uf_union(L, p, q);
  }
}

// grid pixel_blocks * n_frames (images) or node blocks with pixel_blocks = gridDim.x (graphs: one "frame")
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(int* __restrict__ labels, int* __restrict__ sizes, int64_t n, int blocks_per_frame) {
  const int f = blockIdx.x / blocks_per_frame;
  const int64_t i = (int64_t)(blockIdx.x % blocks_per_frame) * CC_THREADS + threadIdx.x;
  int* L = labels + (int64_t)f * n;
  int root = -1;
  if (i < n && uf_load(L + i) >= 0) {
    root = uf_find(L, (int)i);
    uf_store(L + i, root);                      // a root, so still a valid parent for a find that passes through
  }
  wave_count_roots(sizes + (int64_t)f * n, root);
}

__global__ __launch_bounds__(CC_THREADS) void cc_output_kernel(const int* __restrict__ labels, const int* __restrict__ sizes, int64_t hw,
                                                               int blocks_per_frame, int min_size, uint8_t* __restrict__ out_mask,
                                                               int32_t* __restrict__ out_labels, int32_t* __restrict__ stats) {
  __shared__ int cnt[3];
  const int f = blockIdx.x / blocks_per_frame, t = threadIdx.x;
  const int64_t i = (int64_t)(blockIdx.x % blocks_per_frame) * CC_THREADS + t;
  if (t < 3) cnt[t] = 0;
  __syncthreads();
  const int64_t base = (int64_t)f * hw;
  bool fg = false, root = false, keep = false;
  if (i < hw) {
    const int l = labels[base + i];
    fg = l >= 0;
    keep = fg && sizes[base + l] >= min_size;
    root = fg && l == (int)i;
    out_mask[base + i] = keep ? (uint8_t)255 : (uint8_t)0;
    if (out_labels) out_labels[base + i] = fg ? l + 1 : 0;
  }
  if (stats) {                                  // uniform
    const int nf = (int)__popcll(__ballot(fg)), nr = (int)__popcll(__ballot(root)), nk = (int)__popcll(__ballot(root && keep));
    if ((t & 63) == 0) {
      if (nf) atomicAdd(&cnt[0], nf);
      if (nr) atomicAdd(&cnt[1], nr);
      if (nk) atomicAdd(&cnt[2], nk);
    }
    __syncthreads();
    if (t < 3 && cnt[t]) atomicAdd(stats + f * 4 + 1 + t, cnt[t]);
  }
}

// ---- graphs ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CC_THREADS) void cc_graph_init_kernel(int* __restrict__ label, int* __restrict__ sizes, int64_t n,
                                                                   int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (i == 0) flag[0] = 0;
  if (i < n) {
    label[i] = (int)i;
    sizes[i] = 0;
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_graph_union_kernel(int* __restrict__ label, int64_t n, const int32_t* __restrict__ edges,
                                                                    int64_t n_edges, int32_t* __restrict__ flag) {
  const int64_t e = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (e >= n_edges) return;
  const int a = edges[2 * e], b = edges[2 * e + 1];
  if (a < 0 || a >= n || b < 0 || b >= n) {     // never followed: the labels stay those of the valid edges
    atomicOr(flag, 1);
    return;
  }
  if (a != b) uf_union(label, a, b);
}

__global__ __launch_bounds__(CC_THREADS) void cc_graph_size_kernel(const int* __restrict__ label, const int* __restrict__ sizes, int64_t n,
                                                                   int32_t* __restrict__ out_size) {
  const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (i < n) out_size[i] = sizes[label[i]];
}

size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

}  // namespace

// labels int32[n hw] | sizes int32[n hw] | histograms uint32[n 256] | thresholds int32[n], each part 16-byte aligned
extern "C" size_t am_mask_refine_workspace_bytes(int n_frames, int height, int width) {
  if (n_frames < 1 || height < 1 || width < 1) return 0;
  const size_t px = (size_t)n_frames * (size_t)height * (size_t)width;
  return 2 * align16(px * 4) + align16((size_t)n_frames * 256 * 4) + align16((size_t)n_frames * 4);
}

extern "C" int am_mask_refine(const am_mask_refine_args* a, void* stream) {
  AM_CHECK(a != nullptr, "am_mask_refine: null arguments");
  AM_CHECK(a->n_frames >= 1 && a->height >= 1 && a->width >= 1, "am_mask_refine: empty problem (%d frames of %d x %d)", a->n_frames,
           a->height, a->width);
  const int64_t hw = (int64_t)a->height * a->width;
  AM_CHECK(hw < ((int64_t)1 << 31) - 1, "am_mask_refine: %lld pixels per frame do not fit a 32-bit label", (long long)hw);
  AM_CHECK(a->min_size >= 0, "am_mask_refine: negative min_size %d", a->min_size);
  AM_CHECK(a->threshold >= -1 && a->threshold <= 255, "am_mask_refine: threshold %d outside -1 .. 255", a->threshold);
  AM_CHECK(a->mask && a->out_mask, "am_mask_refine: null pointer");
  const size_t need = am_mask_refine_workspace_bytes(a->n_frames, a->height, a->width);
  AM_CHECK(a->workspace != nullptr && a->workspace_bytes >= need, "am_mask_refine: workspace of %zu bytes needed, %zu given", need,
           (size_t)a->workspace_bytes);
  AM_CHECK((reinterpret_cast<uintptr_t>(a->workspace) & 15) == 0, "am_mask_refine: the workspace must be 16-byte aligned");
  const int tiles_x = ceil_div(a->width, CC_TILE), tiles_y = ceil_div(a->height, CC_TILE);
  const int64_t tiles = (int64_t)tiles_x * tiles_y;
  const int64_t px_blocks = (hw + CC_THREADS - 1) / CC_THREADS;
  const int64_t border = (int64_t)(tiles_x - 1) * a->height + (int64_t)(tiles_y - 1) * a->width;
  const int64_t border_blocks = (border + CC_THREADS - 1) / CC_THREADS;
  const int64_t grid_max = ((int64_t)1 << 31) - 1;
  AM_CHECK(tiles * a->n_frames <= grid_max && px_blocks * a->n_frames <= grid_max && border_blocks * a->n_frames <= grid_max &&
               a->n_frames <= 65535,
           "am_mask_refine: %d frames of %d x %d are more than one launch covers", a->n_frames, a->height, a->width);

  const size_t px = (size_t)a->n_frames * (size_t)hw;
  char* ws = reinterpret_cast<char*>(a->workspace);
  int* labels = reinterpret_cast<int*>(ws);
  int* sizes = reinterpret_cast<int*>(ws + align16(px * 4));
  uint32_t* hist = reinterpret_cast<uint32_t*>(ws + 2 * align16(px * 4));
  int32_t* thr = reinterpret_cast<int32_t*>(ws + 2 * align16(px * 4) + align16((size_t)a->n_frames * 256 * 4));
  hipStream_t st = (hipStream_t)stream;
  if (a->threshold < 0) {
    const int64_t nh = (int64_t)a->n_frames * 256;
    hipLaunchKernelGGL(cc_zero_kernel, dim3((unsigned)((nh + CC_THREADS - 1) / CC_THREADS)), dim3(CC_THREADS), 0, st, hist, nh);
    const int64_t chunks = (hw + (int64_t)CC_THREADS * CC_HIST_CHUNK - 1) / ((int64_t)CC_THREADS * CC_HIST_CHUNK);
    const int hb = (int)(chunks < CC_HIST_MAX_BLOCKS ? chunks : CC_HIST_MAX_BLOCKS);
    hipLaunchKernelGGL(cc_hist_kernel, dim3(hb, a->n_frames), dim3(CC_THREADS), 0, st, a->mask, hw, hist);
  }
  hipLaunchKernelGGL(cc_otsu_kernel, dim3(a->n_frames), dim3(64), 0, st, hist, hw, (int)a->threshold, thr, a->out_stats);
  hipLaunchKernelGGL(cc_tile_kernel, dim3((unsigned)(tiles * a->n_frames)), dim3(CC_THREADS), 0, st, a->mask, (int)a->height, (int)a->width,
                     tiles_x, (int)tiles, thr, labels, sizes);
  if (border > 0)
    hipLaunchKernelGGL(cc_merge_kernel, dim3((unsigned)(border_blocks * a->n_frames)), dim3(CC_THREADS), 0, st, labels, (int)a->height,
                       (int)a->width, tiles_x, (int)border, (int)border_blocks);
  hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)(px_blocks * a->n_frames)), dim3(CC_THREADS), 0, st, labels, sizes, hw, (int)px_blocks);
  hipLaunchKernelGGL(cc_output_kernel, dim3((unsigned)(px_blocks * a->n_frames)), dim3(CC_THREADS), 0, st, labels, sizes, hw, (int)px_blocks,
                     (int)a->min_size, a->out_mask, a->out_labels, a->out_stats);
  AM_HIP(hipGetLastError());
  return AM_OK;
}

// sizes int32[n_nodes]: the adds land here, so that out_size is only ever written
extern "C" size_t am_graph_components_workspace_bytes(int64_t n_nodes, int64_t n_edges) {
  (void)n_edges;
  if (n_nodes < 1) return 0;
  return align16((size_t)n_nodes * 4);
}

extern "C" int am_graph_components(const am_graph_args* a, void* stream) {
  AM_CHECK(a != nullptr, "am_graph_components: null arguments");
  AM_CHECK(a->n_nodes >= 1 && a->n_nodes < ((int64_t)1 << 31) - 1, "am_graph_components: %lld nodes outside 1 .. 2^31 - 2",
           (long long)a->n_nodes);
  AM_CHECK(a->n_edges >= 0 && a->n_edges < ((int64_t)1 << 38), "am_graph_components: %lld edges outside 0 .. 2^38", (long long)a->n_edges);
  AM_CHECK(a->out_label && a->out_flag && (a->n_edges == 0 || a->edges), "am_graph_components: null pointer");
  const size_t need = am_graph_components_workspace_bytes(a->n_nodes, a->n_edges);
  AM_CHECK(a->workspace != nullptr && a->workspace_bytes >= need, "am_graph_components: workspace of %zu bytes needed, %zu given", need,
           (size_t)a->workspace_bytes);
  AM_CHECK((reinterpret_cast<uintptr_t>(a->workspace) & 15) == 0, "am_graph_components: the workspace must be 16-byte aligned");
  int* sizes = reinterpret_cast<int*>(a->workspace);
  hipStream_t st = (hipStream_t)stream;
  const unsigned node_blocks = (unsigned)((a->n_nodes + CC_THREADS - 1) / CC_THREADS);
  hipLaunchKernelGGL(cc_graph_init_kernel, dim3(node_blocks), dim3(CC_THREADS), 0, st, a->out_label, sizes, a->n_nodes, a->out_flag);
  if (a->n_edges > 0)
    hipLaunchKernelGGL(cc_graph_union_kernel, dim3((unsigned)((a->n_edges + CC_THREADS - 1) / CC_THREADS)), dim3(CC_THREADS), 0, st,
                       a->out_label, a->n_nodes, a->edges, a->n_edges, a->out_flag);
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(node_blocks), dim3(CC_THREADS), 0, st, a->out_label, sizes, a->n_nodes, (int)node_blocks);
  if (a->out_size)
    hipLaunchKernelGGL(cc_graph_size_kernel, dim3(node_blocks), dim3(CC_THREADS), 0, st, a->out_label, sizes, a->n_nodes, a->out_size);
  AM_HIP(hipGetLastError());
  return AM_OK;
}
