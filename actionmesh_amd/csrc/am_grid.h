// What the two iso-surface methods share (am_isosurface.hip, am_dualcubes.hip): the sample grid of include/actionmesh_amd.h ("Grid."),
// what "finite" and "inside" mean, the tile walk of the two classifying kernels, the index arithmetic of a point and of a cell's
// corners, the edge-crossing interpolation - whose association order is part of the bit-exact contract -, the size limit, the launch
// arithmetic and the host checks.  Everything sits in the unnamed namespace, next to the kernels of the source that includes it.
#pragma once
#include "am_common.h"

#pragma clang fp contract(off)      // the helpers below too, whatever flags the file is built with

namespace {

constexpr int GRID_THREADS = 256;                                          // every kernel: blocks of 256
constexpr int64_t GRID_MAX = ((int64_t)1 << 31) - 1;                       // points, vertices, triangles
constexpr int TILE_I = 8, TILE_J = 8, TILE_K = 64;                         // points of a tile_walk tile; k is the contiguous axis
constexpr int HALO_I = TILE_I + 1, HALO_J = TILE_J + 1, HALO_K = TILE_K + 1;
constexpr int HALO_POINTS = HALO_I * HALO_J * HALO_K;

unsigned grid_blocks(int64_t n) { return (unsigned)((n + GRID_THREADS - 1) / GRID_THREADS); }

struct grid_view {
  int64_t nx, ny, nz;
  double level;
  int inside_above;
};

// bit 0: the value is finite; bit 1: it is finite and inside
__device__ __forceinline__ uint32_t point_state(float v, double level, int inside_above) {
  if (!(fabsf(v) <= 3.402823466e+38f)) return 0u;                 // NaN and both infinities fail the comparison
  const double d = (double)v;
  const bool in = inside_above ? d > level : d < level;
  return in ? 3u : 1u;
}

// One block of GRID_THREADS per TILE_I x TILE_J x TILE_K tile of points, blockIdx (k, j, i): the tile and its one-point halo on the
// high sides go through LDS as one state byte per point, so every value is fetched about once (9 * 9 * 65 / 4096 = 1.29 with the
// halo, most of which the L2 serves); then cell(p, c) for every point p of the tile inside the grid, c.s the states of the eight
// corners of the cell that starts there, corner m = di << 2 | dj << 1 | dk - by value: am_iso_classify is 2 % slower when its
// callable reads them through a reference.  A point outside the grid is "not evaluated".
struct cell_states {
  uint32_t s[8];
};
template <typename Cell>
__device__ __forceinline__ void tile_walk(const grid_view& g, const float* __restrict__ values, Cell cell) {
  __shared__ uint8_t state[HALO_POINTS];
  const int64_t i0 = (int64_t)blockIdx.z * TILE_I, j0 = (int64_t)blockIdx.y * TILE_J, k0 = (int64_t)blockIdx.x * TILE_K;
  for (int e = threadIdx.x; e < HALO_POINTS; e += GRID_THREADS) {
    const int li = e / (HALO_J * HALO_K), r = e - li * (HALO_J * HALO_K), lj = r / HALO_K, lk = r - lj * HALO_K;
    const int64_t i = i0 + li, j = j0 + lj, k = k0 + lk;
    uint32_t s = 0u;
    if (i < g.nx && j < g.ny && k < g.nz) s = point_state(values[(i * g.ny + j) * g.nz + k], g.level, g.inside_above);
    state[e] = (uint8_t)s;
  }
  __syncthreads();
  const int lk = threadIdx.x % TILE_K, plane = threadIdx.x / TILE_K;
  const int64_t k = k0 + lk;
  if (k >= g.nz) return;
  for (int ij = plane; ij < TILE_I * TILE_J; ij += GRID_THREADS / TILE_K) {
    const int li = ij / TILE_J, lj = ij - li * TILE_J;
    const int64_t i = i0 + li, j = j0 + lj;
    if (i >= g.nx || j >= g.ny) continue;
    cell_states c;
#pragma unroll
    for (int m = 0; m < 8; ++m) c.s[m] = state[((li + (m >> 2)) * HALO_J + (lj + ((m >> 1) & 1))) * HALO_K + (lk + (m & 1))];
    cell((i * g.ny + j) * g.nz + k, c);
  }
}

// point p = (i ny + j) nz + k as (i, j, k); the strides of the three axes; corner m = di << 2 | dj << 1 | dk of the cell that starts
// at p.  The strides are apart from the point: a kernel asks for them where it needs them, behind its checks.
struct grid_point {
  int64_t i, j, k;
};
struct grid_steps {
  int64_t s[3];
};
__device__ __forceinline__ grid_point point_at(int64_t p, int64_t ny, int64_t nz) {
  const int64_t k = p % nz, ij = p / nz, j = ij % ny, i = ij / ny;
  return {i, j, k};
}
__device__ __forceinline__ grid_steps steps_of(int64_t ny, int64_t nz) { return {{ny * nz, nz, 1}}; }
__device__ __forceinline__ int64_t cell_corner(int64_t p, const grid_steps& step, int m) {
  return p + (m >> 2) * step.s[0] + ((m >> 1) & 1) * step.s[1] + (m & 1) * step.s[2];
}

// where the edge from pa (value va) to pb (value vb) crosses the level, one coordinate: t, then d, t d and pa + t d, each rounded on its own
__device__ __forceinline__ double crossing(double level, double va, double vb, double pa, double pb) {
  const double t = (level - va) / (vb - va);
  const double d = pb - pa;
  const double td = t * d;
  return pa + td;
}

// what every entry point checks first, in its own name
int check_grid(const char* who, int64_t nx, int64_t ny, int64_t nz) {
  AM_CHECK(nx >= 2 && ny >= 2 && nz >= 2, "%s: a grid of %lld x %lld x %lld points; every axis needs at least 2", who, (long long)nx,
           (long long)ny, (long long)nz);
  AM_CHECK(nx <= GRID_MAX && ny <= GRID_MAX && nz <= GRID_MAX && nx * ny <= GRID_MAX && nx * ny * nz <= GRID_MAX,
           "%s: a grid of %lld x %lld x %lld points has more than 2^31 - 1", who, (long long)nx, (long long)ny, (long long)nz);
  return AM_OK;
}
int check_level(const char* who, double level) {
  AM_CHECK(level == level && level - level == 0.0, "%s: the level is not finite", who);
  return AM_OK;
}
// n_vertices, n_triangles: `what` is "vertices" or "triangles"
int check_count(const char* who, const char* what, int64_t n) {
  AM_CHECK(n >= 1 && n <= GRID_MAX, "%s: %lld %s outside 1 .. 2^31 - 1", who, (long long)n, what);
  return AM_OK;
}
// the launch grid of tile_walk
int tile_blocks(const char* who, int64_t nx, int64_t ny, int64_t nz, dim3& blocks) {
  const int64_t bi = (nx + TILE_I - 1) / TILE_I, bj = (ny + TILE_J - 1) / TILE_J, bk = (nz + TILE_K - 1) / TILE_K;
  AM_CHECK(bi <= 65535 && bj <= 65535, "%s: more than 65535 tiles along an axis", who);
  blocks = dim3((unsigned)bk, (unsigned)bj, (unsigned)bi);
  return AM_OK;
}

}  // namespace
