// Exact nearest-neighbour search through a uniform grid: am_nn_search's results bit for bit (the same d2 arithmetic, ties to the
// lowest index, index -1 / d2 +inf when no distance is finite) while only the points of a growing cube of cells are evaluated.
// The contract - the grid's arrays, the cell arithmetic operation by operation, the ring walk, its stopping rule and the proof that
// the rule is exact - is include/actionmesh_amd.h's; this file is built with -ffp-contract=off and without SLP packing.
//
//   am_nn_grid_cells (two memsets, two launches):
//     minmax   per cloud, the extrema of the finite points: registers -> wave shuffles -> one integer atomicMin / atomicMax per wave
//              on the order-preserving map of the bit patterns (no float atomics: the result does not depend on scheduling)
//     cell     one thread per point: every thread derives the frame from the six extrema (the same few operations, so no third
//              launch), thread 0 stores it, and each writes its point's cell
//   [the caller sorts the cells: any stable argsort]
//   am_nn_grid_build (three memsets, two launches):
//     fill     one thread per sorted position: compares the `order` entry with its bound, copies the point as a 16-byte record
//              { x, y, z, index bits }, stages its cell, and folds the finite points into the per-axis slab extrema (integer atomics)
//     start    one thread per cell: cell_start[c] = lower bound of c in the staged cells (a binary search: whatever the staged
//              values are, the result lies in [0, n_points]); three threads per cloud turn the slab extrema into the suffix-minimum
//              and prefix-maximum tables
//   am_nn_grid_search (one memset, one launch): one lane per query, about 2048 workgroups with a grid stride, no LDS.  Lanes take
//     queries in `query_order` (the query cloud's own cell order: a wave then walks the same cells and its loads coalesce).  A row
//     of cells along x is ONE range of the sorted copy, so a ring is scanned as (2r + 1)^2 rows: full rows on the shell's four
//     faces, the two end cells elsewhere.  Each range is two cell_start loads, compared with 0 <= begin <= end <= n_points before
//     any record is loaded, then 16-byte loads of the records.
#include "am_points.h"

namespace {

constexpr int GRID_THREADS = 256;
constexpr int GRID_SEARCH_BLOCKS = 2048;
constexpr uint32_t MAP_NONE = 0xffffffffu;       // the minimum's identity; the map of no finite value

// order-preserving map float -> uint32 (the IEEE total order on non-NaN values, -0 below +0) and its inverse
__device__ __forceinline__ uint32_t fmap(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float funmap(uint32_t u) { return __uint_as_float((u >> 31) ? (u & 0x7fffffffu) : ~u); }

// the header's clamped cell along one axis (step 2 of the search), of a point and of a query alike: only an in-range t is converted
__device__ __forceinline__ int cell_axis(float v, float lo, float inv, int G) {
  int c = 0;
  if (inv != 0.f) {
    const float d = v - lo;
    const float t = d * inv;
    if (t >= (float)G)
      c = G - 1;
    else if (t >= 0.f)
      c = (int)floorf(t);
  }
  return c;
}
// the header's cell of a point: the extra cell `ncell` for a non-finite one
__device__ __forceinline__ int cell_of(float x, float y, float z, const float* __restrict__ frame, int G, int ncell) {
  if (!finite3(x, y, z)) return ncell;
  const int c0 = cell_axis(x, frame[0], frame[4], G), c1 = cell_axis(y, frame[1], frame[5], G), c2 = cell_axis(z, frame[2], frame[6], G);
  return (c2 * G + c1) * G + c0;
}

// extrema words of the workspace: [min: batch x 4][max: batch x 4][slab min: batch x 3 x G][slab max: batch x 3 x G][cells: batch x P]
struct GridScratch {
  uint32_t *mn, *mx, *smn, *smx;
  int32_t* cells;
};
__host__ __device__ inline size_t pad16(size_t n) { return (n + 15) / 16 * 16; }
GridScratch grid_scratch(void* ws, int batch, int G) {
  GridScratch s;
  s.mn = reinterpret_cast<uint32_t*>(ws);
  s.mx = s.mn + (size_t)batch * 4;
  s.smn = s.mx + (size_t)batch * 4;
  s.smx = s.smn + (size_t)batch * 3 * G;
  s.cells = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(ws) + pad16(sizeof(uint32_t) * (size_t)batch * (8 + 6 * (size_t)G)));
  return s;
}

// grid (blocks, batch)
__global__ __launch_bounds__(GRID_THREADS) void grid_minmax_kernel(const float* __restrict__ pts, int64_t P, int64_t bstride,
                                                                   uint32_t* __restrict__ mn, uint32_t* __restrict__ mx) {
  const int b = blockIdx.y;
  pts += (int64_t)b * bstride;
  uint32_t lo[3] = {MAP_NONE, MAP_NONE, MAP_NONE}, hi[3] = {0u, 0u, 0u};
  for (int64_t i = (int64_t)blockIdx.x * GRID_THREADS + threadIdx.x; i < P; i += (int64_t)gridDim.x * GRID_THREADS) {
    const float x = pts[i * 3], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
    if (!finite3(x, y, z)) continue;
    const uint32_t m[3] = {fmap(x), fmap(y), fmap(z)};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      lo[k] = m[k] < lo[k] ? m[k] : lo[k];
      hi[k] = m[k] > hi[k] ? m[k] : hi[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t ol = __shfl_xor(lo[k], off, 64), oh = __shfl_xor(hi[k], off, 64);
      lo[k] = ol < lo[k] ? ol : lo[k];
      hi[k] = oh > hi[k] ? oh : hi[k];
    }
    if ((threadIdx.x & 63) == 0 && lo[k] != MAP_NONE) {
      atomicMin(mn + b * 4 + k, lo[k]);
      atomicMax(mx + b * 4 + k, hi[k]);
    }
  }
}

// grid (point blocks, batch)
__global__ __launch_bounds__(GRID_THREADS) void grid_cell_kernel(const float* __restrict__ pts, int64_t P, int64_t bstride, int G,
                                                                 const uint32_t* __restrict__ mn, const uint32_t* __restrict__ mx,
                                                                 float* __restrict__ frame_out, int32_t* __restrict__ out_cell) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * GRID_THREADS + threadIdx.x;
  if (i >= P) return;
  float frame[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (mn[b * 4] != MAP_NONE) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float lo = funmap(mn[b * 4 + k]), hi = funmap(mx[b * 4 + k]);
      const float ext = hi - lo;
      // a double quotient of two floats, rounded to float, is the correctly rounded float quotient (53 >= 2 * 24 + 2 bits)
      const float q = (float)((double)G / (double)ext);
      frame[k] = lo;
      frame[4 + k] = (ext == 0.f || !isfinite(q)) ? 0.f : q;
    }
  }
  if (i == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) frame_out[b * 8 + k] = frame[k];
  }
  const float* p = pts + (int64_t)b * bstride + i * 3;
  out_cell[(int64_t)b * P + i] = cell_of(p[0], p[1], p[2], frame, G, G * G * G);
}

// grid (point blocks, batch)
__global__ __launch_bounds__(GRID_THREADS) void grid_fill_kernel(const float* __restrict__ pts, int64_t P, int64_t bstride, int G,
                                                                 const float* __restrict__ frames, const int32_t* __restrict__ order,
                                                                 float4* __restrict__ sorted, int32_t* __restrict__ cells,
                                                                 uint32_t* __restrict__ smn, uint32_t* __restrict__ smx,
                                                                 int32_t* __restrict__ flag) {
  const int b = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * GRID_THREADS + threadIdx.x;
  if (i >= P) return;
  const int ncell = G * G * G;
  const int32_t o = order[(int64_t)b * P + i];
  float4 rec = {__uint_as_float(0x7fc00000u), __uint_as_float(0x7fc00000u), __uint_as_float(0x7fc00000u), __int_as_float(-1)};
  int c = ncell;
  if ((uint32_t)o >= (uint64_t)P) {                 // compared with its bound before it addresses a point
    atomicOr(flag, AM_NN_GRID_BAD_ORDER);
  } else {
    const float* p = pts + (int64_t)b * bstride + (int64_t)o * 3;
    rec = {p[0], p[1], p[2], __int_as_float(o)};
    const float* frame = frames + b * 8;
    c = cell_of(rec.x, rec.y, rec.z, frame, G, ncell);
    if (c < ncell) {
      const int ck[3] = {c % G, (c / G) % G, c / (G * G)};
      const uint32_t m[3] = {fmap(rec.x), fmap(rec.y), fmap(rec.z)};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        atomicMin(smn + ((size_t)b * 3 + k) * G + ck[k], m[k]);
        atomicMax(smx + ((size_t)b * 3 + k) * G + ck[k], m[k]);
      }
    }
  }
  sorted[(int64_t)b * P + i] = rec;
  cells[(int64_t)b * P + i] = c;
}

// grid (cell blocks, batch)
__global__ __launch_bounds__(GRID_THREADS) void grid_start_kernel(int64_t P, int G, const int32_t* __restrict__ cells,
                                                                  const uint32_t* __restrict__ smn, const uint32_t* __restrict__ smx,
                                                                  int32_t* __restrict__ cell_start, float* __restrict__ slabs) {
  const int b = blockIdx.y;
  const int64_t ncell = (int64_t)G * G * G;
  const int64_t c = (int64_t)blockIdx.x * GRID_THREADS + threadIdx.x;
  if (c < ncell + 2) {
    const int32_t* cs = cells + (int64_t)b * P;
    int64_t lo = 0, hi = P;
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (cs[mid] < c)
        lo = mid + 1;
      else
        hi = mid;
    }
    cell_start[(int64_t)b * (ncell + 2) + c] = (int32_t)lo;
  }
  if (c < 3) {            // axis c of this cloud: the suffix minimum and the prefix maximum over the slabs
    const int k = (int)c;
    const uint32_t* mn = smn + ((size_t)b * 3 + k) * G;
    const uint32_t* mx = smx + ((size_t)b * 3 + k) * G;
    float* smin = slabs + ((size_t)b * 6 + k) * G;
    float* pmax = slabs + ((size_t)b * 6 + 3 + k) * G;
    uint32_t run = MAP_NONE;
    for (int j = G - 1; j >= 0; --j) {
      run = mn[j] < run ? mn[j] : run;
      smin[j] = run == MAP_NONE ? INFINITY : funmap(run);
    }
    run = 0u;
    for (int j = 0; j < G; ++j) {
      run = mx[j] > run ? mx[j] : run;
      pmax[j] = run == 0u ? -INFINITY : funmap(run);
    }
  }
}

template <typename T> struct Best { T d2; int32_t index; };

// the records of cells first .. last (one row along x): false, with the flag raised, when the range is not inside the sorted copy
template <typename T>
__device__ __forceinline__ bool scan_cells(const int32_t* __restrict__ cs, const float4* __restrict__ srt, int64_t P, int first, int last,
                                           T qx, T qy, T qz, Best<T>& best, int32_t* __restrict__ flag) {
#pragma clang fp contract(off)
  const int32_t s = cs[first], e = cs[last + 1];
  if (s < 0 || e < s || (int64_t)e > P) {
    atomicOr(flag, AM_NN_GRID_BAD_CELL_START);
    return false;
  }
  for (int32_t j = s; j < e; ++j) {
    const float4 p = srt[j];
    const int32_t idx = __float_as_int(p.w);
    if ((uint32_t)idx >= (uint64_t)P) {
      atomicOr(flag, AM_NN_GRID_BAD_INDEX);
      continue;
    }
    take_any_order(best.d2, best.index, dist2(qx, qy, qz, (T)p.x, (T)p.y, (T)p.z), idx);
  }
  return true;
}

template <typename T>
__global__ __launch_bounds__(GRID_THREADS) void grid_search_kernel(am_nn_grid g, const float* __restrict__ qry, int64_t Q, int64_t q_bstride,
                                                                   int batch, const int32_t* __restrict__ qorder, int64_t qo_bstride,
                                                                   T* __restrict__ out_d2, int32_t* __restrict__ out_idx,
                                                                   int32_t* __restrict__ flag) {
#pragma clang fp contract(off)
  const int G = g.cells;
  const int64_t P = g.n_points, ncell = (int64_t)G * G * G, total = (int64_t)batch * Q;
  for (int64_t item = (int64_t)blockIdx.x * GRID_THREADS + threadIdx.x; item < total; item += (int64_t)gridDim.x * GRID_THREADS) {
    const int64_t b = item / Q;
    int64_t qi = item - b * Q;
    if (qorder) {
      const int32_t o = qorder[b * qo_bstride + qi];
      if ((uint32_t)o >= (uint64_t)Q) {              // no position to write: the entry is skipped, the flag says so
        atomicOr(flag, AM_NN_GRID_BAD_QUERY_ORDER);
        continue;
      }
      qi = o;
    }
    const int64_t gb = g.batch == 1 ? 0 : b;
    const float* frame = g.frame + gb * 8;
    const float* slabs = g.slabs + gb * 6 * G;
    const int32_t* cs = g.cell_start + gb * (ncell + 2);
    const float4* srt = reinterpret_cast<const float4*>(g.sorted) + gb * P;
    const float* qp = qry + b * q_bstride + qi * 3;
    const float qf[3] = {qp[0], qp[1], qp[2]};
    Best<T> best = {(T)INFINITY, -1};
    if (finite3(qf[0], qf[1], qf[2])) {
      int c[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) c[k] = cell_axis(qf[k], frame[k], frame[4 + k], G);
      const T q[3] = {(T)qf[0], (T)qf[1], (T)qf[2]};
      bool ok = true;
      for (int r = 0; r < G && ok; ++r) {                                  // at most G rings
        const int x0 = c[0] - r > 0 ? c[0] - r : 0, x1 = c[0] + r < G - 1 ? c[0] + r : G - 1;
        const int y0 = c[1] - r > 0 ? c[1] - r : 0, y1 = c[1] + r < G - 1 ? c[1] + r : G - 1;
        const int z0 = c[2] - r > 0 ? c[2] - r : 0, z1 = c[2] + r < G - 1 ? c[2] + r : G - 1;
        for (int z = z0; z <= z1 && ok; ++z)
          for (int y = y0; y <= y1 && ok; ++y) {
            const int row = (z * G + y) * G;
            if (z == c[2] - r || z == c[2] + r || y == c[1] - r || y == c[1] + r) {
              ok = scan_cells<T>(cs, srt, P, row + x0, row + x1, q[0], q[1], q[2], best, flag);
            } else {                                                         // r >= 1 here: the two end cells of the row
              if (c[0] - r >= 0) ok = scan_cells<T>(cs, srt, P, row + c[0] - r, row + c[0] - r, q[0], q[1], q[2], best, flag);
              if (ok && c[0] + r < G) ok = scan_cells<T>(cs, srt, P, row + c[0] + r, row + c[0] + r, q[0], q[1], q[2], best, flag);
            }
          }
        if (!ok) break;
        T gmin = (T)INFINITY;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int hi = c[k] + r + 1, lo = c[k] - r - 1;
          if (hi < G) {
            const T gg = (T)slabs[k * G + hi] - q[k];
            if (gg < gmin) gmin = gg;
          }
          if (lo >= 0) {
            const T gg = q[k] - (T)slabs[(3 + k) * G + lo];
            if (gg < gmin) gmin = gg;
          }
        }
        if (!(gmin < (T)INFINITY)) break;            // every side exhausted: no finite point lies outside the cube
        if (best.d2 < gmin * gmin) break;
      }
      if (!ok) best = {(T)INFINITY, -1};
    }
    out_d2[b * Q + qi] = best.d2;
    out_idx[b * Q + qi] = best.index;
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int grid_check(const char* who, const am_nn_grid* g, bool building) {
  AM_CHECK(g->cells >= 1 && g->cells <= AM_NN_GRID_MAX_CELLS, "%s: %d cells per axis outside 1 .. %d", who, g->cells, AM_NN_GRID_MAX_CELLS);
  AM_TRY(check_cloud(who, g->batch, g->n_points, "points", 'y'));
  AM_CHECK(g->frame && g->slabs && g->cell_start && g->sorted && (g->order || !building), "%s: null grid pointer", who);
  AM_CHECK(aligned16(g->frame) && aligned16(g->slabs) && aligned16(g->cell_start) && aligned16(g->order) && aligned16(g->sorted),
           "%s: the grid's arrays must be 16-byte aligned", who);
  return AM_OK;
}

int build_check(const char* who, const am_nn_grid_build_args* a) {
  AM_CHECK(a != nullptr, "%s: null arguments", who);
  AM_TRY(grid_check(who, &a->grid, true));
  AM_CHECK(a->points != nullptr, "%s: null pointer", who);
  AM_CHECK(a->points_bstride == 0 || a->points_bstride >= 3 * a->grid.n_points, "%s: batch stride %lld below 3 * %lld points", who,
           (long long)a->points_bstride, (long long)a->grid.n_points);
  AM_TRY(check_workspace(who, a->workspace, (size_t)a->workspace_bytes, am_nn_grid_workspace_bytes(a->grid.n_points, a->grid.batch, a->grid.cells)));
  AM_CHECK(aligned16(a->workspace), "%s: the workspace must be 16-byte aligned", who);
  return AM_OK;
}

template <typename T>
void search_launch(const am_nn_grid_search_args* a, hipStream_t st) {
  const int64_t total = (int64_t)a->batch * a->n_queries;
  const int64_t blocks = (total + GRID_THREADS - 1) / GRID_THREADS;
  hipLaunchKernelGGL((grid_search_kernel<T>), dim3((unsigned)(blocks < GRID_SEARCH_BLOCKS ? blocks : GRID_SEARCH_BLOCKS)), dim3(GRID_THREADS),
                     0, st, a->grid, a->queries, a->n_queries, a->queries_bstride, (int)a->batch, a->query_order, a->query_order_bstride,
                     reinterpret_cast<T*>(a->out_d2), a->out_index, a->out_flag);
}

}  // namespace

extern "C" size_t am_nn_grid_bytes(int64_t n_points, int batch, int cells) {
  if (!cloud_ok(batch, n_points) || cells < 1 || cells > AM_NN_GRID_MAX_CELLS) return 0;
  const size_t B = (size_t)batch, P = (size_t)n_points, G = (size_t)cells;
  return pad16(B * 8 * sizeof(float)) + pad16(B * 6 * G * sizeof(float)) + pad16(B * (G * G * G + 2) * sizeof(int32_t)) +
         pad16(B * P * sizeof(int32_t)) + pad16(B * P * 4 * sizeof(float));
}

extern "C" size_t am_nn_grid_workspace_bytes(int64_t n_points, int batch, int cells) {
  if (!cloud_ok(batch, n_points) || cells < 1 || cells > AM_NN_GRID_MAX_CELLS) return 0;
  return pad16(sizeof(uint32_t) * (size_t)batch * (8 + 6 * (size_t)cells)) + pad16(sizeof(int32_t) * (size_t)batch * (size_t)n_points);
}

extern "C" int am_nn_grid_cells(const am_nn_grid_build_args* a, void* stream) {
  AM_TRY(build_check("am_nn_grid_cells", a));
  AM_CHECK(a->out_cell != nullptr, "am_nn_grid_cells: null pointer");
  const am_nn_grid& g = a->grid;
  hipStream_t st = (hipStream_t)stream;
  const GridScratch s = grid_scratch(a->workspace, g.batch, g.cells);
  AM_HIP(hipMemsetAsync(s.mn, 0xff, sizeof(uint32_t) * 4 * (size_t)g.batch, st));
  AM_HIP(hipMemsetAsync(s.mx, 0, sizeof(uint32_t) * 4 * (size_t)g.batch, st));
  const int pblocks = ceil_div(g.n_points, GRID_THREADS);
  hipLaunchKernelGGL(grid_minmax_kernel, dim3(pblocks < 64 ? pblocks : 64, g.batch), dim3(GRID_THREADS), 0, st, a->points, g.n_points,
                     a->points_bstride, s.mn, s.mx);
  hipLaunchKernelGGL(grid_cell_kernel, dim3(pblocks, g.batch), dim3(GRID_THREADS), 0, st, a->points, g.n_points, a->points_bstride, g.cells,
                     s.mn, s.mx, g.frame, a->out_cell);
  AM_HIP(hipGetLastError());
  return AM_OK;
}

extern "C" int am_nn_grid_build(const am_nn_grid_build_args* a, void* stream) {
  AM_TRY(build_check("am_nn_grid_build", a));
  AM_CHECK(a->out_flag != nullptr, "am_nn_grid_build: null pointer");
  const am_nn_grid& g = a->grid;
  hipStream_t st = (hipStream_t)stream;
  const GridScratch s = grid_scratch(a->workspace, g.batch, g.cells);
  const size_t slab_bytes = sizeof(uint32_t) * 3 * (size_t)g.cells * (size_t)g.batch;
  AM_HIP(hipMemsetAsync(a->out_flag, 0, sizeof(int32_t), st));
  AM_HIP(hipMemsetAsync(s.smn, 0xff, slab_bytes, st));
  AM_HIP(hipMemsetAsync(s.smx, 0, slab_bytes, st));
  const int64_t ncell = (int64_t)g.cells * g.cells * g.cells;
  hipLaunchKernelGGL(grid_fill_kernel, dim3(ceil_div(g.n_points, GRID_THREADS), g.batch), dim3(GRID_THREADS), 0, st, a->points, g.n_points,
                     a->points_bstride, g.cells, g.frame, g.order, reinterpret_cast<float4*>(g.sorted), s.cells, s.smn, s.smx, a->out_flag);
  hipLaunchKernelGGL(grid_start_kernel, dim3(ceil_div(ncell + 2, GRID_THREADS), g.batch), dim3(GRID_THREADS), 0, st, g.n_points, g.cells,
                     s.cells, s.smn, s.smx, g.cell_start, g.slabs);
  AM_HIP(hipGetLastError());
  return AM_OK;
}

extern "C" int am_nn_grid_search(const am_nn_grid_search_args* a, void* stream) {
  AM_CHECK(a != nullptr, "am_nn_grid_search: null arguments");
  AM_TRY(grid_check("am_nn_grid_search", &a->grid, false));
  AM_TRY(check_cloud("am_nn_grid_search", a->batch, a->n_queries, "queries", 0));       // one lane per query: the batch is no grid axis
  AM_CHECK(a->grid.batch == a->batch || a->grid.batch == 1, "am_nn_grid_search: %d grids for a batch of %d (one shared grid or one each)",
           a->grid.batch, a->batch);
  AM_CHECK(a->queries && a->out_index && a->out_d2 && a->out_flag, "am_nn_grid_search: null pointer");
  AM_CHECK(a->queries_bstride == 0 || a->queries_bstride >= 3 * a->n_queries, "am_nn_grid_search: batch stride %lld below 3 * %lld queries",
           (long long)a->queries_bstride, (long long)a->n_queries);
  AM_CHECK(a->query_order == nullptr || a->query_order_bstride == 0 || a->query_order_bstride >= a->n_queries,
           "am_nn_grid_search: query_order stride %lld below %lld queries", (long long)a->query_order_bstride, (long long)a->n_queries);
  hipStream_t st = (hipStream_t)stream;
  AM_HIP(hipMemsetAsync(a->out_flag, 0, sizeof(int32_t), st));
  if (a->precise)
    search_launch<double>(a, st);
  else
    search_launch<float>(a, st);
  AM_HIP(hipGetLastError());
  return AM_OK;
}
