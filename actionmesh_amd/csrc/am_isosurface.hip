// Iso-surface extraction: marching tetrahedra on a regular grid (actionmesh_amd/isosurface.py), which stands in for the `diso` dual
// marching cubes behind TripoSG's hierarchical_extract_geometry (actionmesh/external/triposg.py:13, 193-199).  The contract is
// include/actionmesh_amd.h's; the interpolation is fp64, every operation rounded on its own (the file is built with
// -ffp-contract=off), so masks, counts, vertices and faces are compared bit for bit with a numpy restatement.
//
//   am_iso_classify    one block per 8 x 8 x 64 tile of points (am_grid.h's tile_walk): per point the mask of crossing edges that
//                      start there, per cell the number of triangles
//   am_iso_vertices    one thread per point: a point with a non-zero mask writes its vertices at vertex_offset[p] + rank of the bit
//   am_iso_triangles   one thread per point: a cell with a non-zero count writes its faces at tri_offset[p]
// No atomics but the OR into the flag word, no hash table: the order of vertices and faces is fixed by the two prefix sums the caller
// makes.  No offset or index read from memory is used as an address before it has been compared with its bound.
// From am_grid.h, shared with am_dualcubes.hip: the grid and point_state, the tile walk, the index arithmetic of a point and of a
// cell's corners, the crossing interpolation, the launch arithmetic and the host checks.
#include "am_grid.h"

namespace {

// the corners c0 .. c3 of Kuhn tetrahedron t as offset codes (di << 2 | dj << 1 | dk): c0 = 000, c1 = c0 + e_pi0, c2 = c1 + e_pi1,
// c3 = 111, for the t-th permutation pi of the axes (i, j, k) in lexicographic order
__constant__ uint8_t ISO_CORNER[6][4] = {{0, 4, 6, 7}, {0, 4, 5, 7}, {0, 2, 6, 7}, {0, 2, 3, 7}, {0, 1, 5, 7}, {0, 1, 3, 7}};
// an odd permutation mirrors the tetrahedron: its polygons are the reversed ones
__constant__ uint8_t ISO_PARITY[6] = {0, 1, 1, 0, 0, 1};
// [parity][inside mask of (c0 .. c3)][2 triangles x 3 vertices]: a vertex is the edge between corners a < b as 4 a + b, 255 = none.
// The rule (header): one inside corner a -> (a, o) over the outside corners ascending; three -> (i, o) over the inside corners
// ascending; two -> (i0,o0) (i0,o1) (i1,o1) (i1,o0) split along its first and third vertex; reversed behind the first vertex when
// the normal would point from the outside corners to the inside ones.
__constant__ uint8_t ISO_CASE[2][16][6] = {
    {{255, 255, 255, 255, 255, 255}, {1, 2, 3, 255, 255, 255}, {1, 7, 6, 255, 255, 255}, {2, 3, 7, 2, 7, 6},
     {2, 6, 11, 255, 255, 255},      {1, 6, 11, 1, 11, 3},     {1, 7, 11, 1, 11, 2},     {3, 7, 11, 255, 255, 255},
     {3, 11, 7, 255, 255, 255},      {1, 2, 11, 1, 11, 7},     {1, 3, 11, 1, 11, 6},     {2, 11, 6, 255, 255, 255},
     {2, 6, 7, 2, 7, 3},             {1, 6, 7, 255, 255, 255}, {1, 3, 2, 255, 255, 255}, {255, 255, 255, 255, 255, 255}},
    {{255, 255, 255, 255, 255, 255}, {1, 3, 2, 255, 255, 255}, {1, 6, 7, 255, 255, 255}, {2, 6, 7, 2, 7, 3},
     {2, 11, 6, 255, 255, 255},      {1, 3, 11, 1, 11, 6},     {1, 2, 11, 1, 11, 7},     {3, 11, 7, 255, 255, 255},
     {3, 7, 11, 255, 255, 255},      {1, 7, 11, 1, 11, 2},     {1, 6, 11, 1, 11, 3},     {2, 6, 11, 255, 255, 255},
     {2, 3, 7, 2, 7, 6},             {1, 7, 6, 255, 255, 255}, {1, 2, 3, 255, 255, 255}, {255, 255, 255, 255, 255, 255}}};

// the triangles of one tetrahedron from the states of its corners: 0 with a non-finite corner
__device__ __forceinline__ uint32_t tet_case(const uint32_t (&s)[8], int t, bool& finite) {
  const uint32_t a = s[0], b = s[ISO_CORNER[t][1]], c = s[ISO_CORNER[t][2]], d = s[7];
  finite = (a & b & c & d & 1u) != 0u;
  return (a >> 1) | (b >> 1) << 1 | (c >> 1) << 2 | (d >> 1) << 3;
}
__device__ __forceinline__ uint32_t case_triangles(uint32_t cs) {
  const int n = __popc(cs);
  return n == 0 || n == 4 ? 0u : (n == 2 ? 2u : 1u);
}

__global__ __launch_bounds__(GRID_THREADS) void iso_classify_kernel(grid_view g, const float* __restrict__ values,
                                                                    uint8_t* __restrict__ out_mask, uint8_t* __restrict__ out_count) {
  tile_walk(g, values, [=](int64_t p, cell_states c) {
    uint32_t mask = 0u;
#pragma unroll
    for (int m = 1; m < 8; ++m)
      if ((c.s[0] & c.s[m] & 1u) && ((c.s[0] ^ c.s[m]) & 2u)) mask |= 1u << (m - 1);
    uint32_t count = 0u;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      bool finite;
      const uint32_t cs = tet_case(c.s, t, finite);
      if (finite) count += case_triangles(cs);
    }
    out_mask[p] = (uint8_t)mask;
    out_count[p] = (uint8_t)count;
  });
}

__global__ __launch_bounds__(GRID_THREADS) void iso_vertices_kernel(grid_view g, const float* __restrict__ values,
                                                                    const uint8_t* __restrict__ mask,
                                                                    const int64_t* __restrict__ vertex_offset, int64_t n_vertices,
                                                                    double ox, double oy, double oz, double sx, double sy, double sz,
                                                                    float* __restrict__ out_vertices, int32_t* flag) {
#pragma clang fp contract(off)
  const int64_t p = (int64_t)blockIdx.x * GRID_THREADS + threadIdx.x;
  if (p >= g.nx * g.ny * g.nz) return;
  const uint32_t mk = mask[p];
  if (mk == 0u) return;
  const int64_t base = vertex_offset[p];
  if (mk > 127u || base < 0 || base > n_vertices - (int64_t)__popc(mk)) {
    atomicOr(flag, mk > 127u ? AM_ISO_BAD_TABLE : AM_ISO_BAD_VERTEX_OFFSET);
    return;
  }
  const grid_point at = point_at(p, g.ny, g.nz);
  const double va = (double)values[p];
  const double pa[3] = {ox + (double)at.i * sx, oy + (double)at.j * sy, oz + (double)at.k * sz};
  int rank = 0;
  for (int m = 1; m < 8; ++m) {
    if (!(mk >> (m - 1) & 1u)) continue;
    const int64_t slot = base + rank++;
    const int64_t bi = at.i + (m >> 2), bj = at.j + ((m >> 1) & 1), bk = at.k + (m & 1);
    if (bi >= g.nx || bj >= g.ny || bk >= g.nz) {               // the mask names an edge that leaves the grid
      atomicOr(flag, AM_ISO_BAD_TABLE);
      continue;
    }
    const double vb = (double)values[(bi * g.ny + bj) * g.nz + bk];
    const double pb[3] = {ox + (double)bi * sx, oy + (double)bj * sy, oz + (double)bk * sz};
    for (int c = 0; c < 3; ++c) out_vertices[slot * 3 + c] = (float)crossing(g.level, va, vb, pa[c], pb[c]);
  }
}

__global__ __launch_bounds__(GRID_THREADS) void iso_triangles_kernel(grid_view g, const float* __restrict__ values,
                                                                     const uint8_t* __restrict__ mask, const uint8_t* __restrict__ count,
                                                                     const int64_t* __restrict__ vertex_offset,
                                                                     const int64_t* __restrict__ tri_offset, int64_t n_vertices,
                                                                     int64_t n_triangles, int32_t* __restrict__ out_faces, int32_t* flag) {
  const int64_t p = (int64_t)blockIdx.x * GRID_THREADS + threadIdx.x;
  if (p >= g.nx * g.ny * g.nz) return;
  const int64_t want = count[p];
  if (want == 0) return;
  const grid_point at = point_at(p, g.ny, g.nz);
  if (want > 12 || at.i + 1 >= g.nx || at.j + 1 >= g.ny || at.k + 1 >= g.nz) {      // a count where no cell starts
    atomicOr(flag, AM_ISO_BAD_TABLE);
    return;
  }
  const int64_t base = tri_offset[p];
  if (base < 0 || base > n_triangles - want) {
    atomicOr(flag, AM_ISO_BAD_TRI_OFFSET);
    return;
  }
  const grid_steps step = steps_of(g.ny, g.nz);
  uint32_t s[8];
  int64_t corner[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    corner[m] = cell_corner(p, step, m);
    s[m] = point_state(values[corner[m]], g.level, g.inside_above);
  }
  int64_t written = 0;
  bool bad_table = false;
  for (int t = 0; t < 6; ++t) {
    bool finite;
    const uint32_t cs = tet_case(s, t, finite);
    if (!finite) continue;
    const uint32_t n = case_triangles(cs);
    for (uint32_t tri = 0; tri < n; ++tri) {
      if (written >= want) {                                      // more triangles than the count reserved room for
        bad_table = true;
        break;
      }
      int32_t idx[3];
      bool ok = true;
      for (int c = 0; c < 3; ++c) {
        const uint32_t e = ISO_CASE[ISO_PARITY[t]][cs][tri * 3 + c];
        const uint32_t ca = ISO_CORNER[t][e >> 2], cb = ISO_CORNER[t][e & 3u];
        const uint32_t m = cb - ca;                               // the corners of a tetrahedron are nested: the offset of the edge
        const int64_t pa = corner[ca];
        const uint32_t mk = mask[pa];
        const int64_t vo = vertex_offset[pa];
        if (!(mk >> (m - 1) & 1u) || mk > 127u) {
          bad_table = true;
          ok = false;
          continue;
        }
        const int64_t rank = __popc(mk & ((1u << (m - 1)) - 1u));
        if (vo < 0 || vo >= n_vertices - rank) {
          atomicOr(flag, AM_ISO_BAD_VERTEX_OFFSET);
          ok = false;
          continue;
        }
        idx[c] = (int32_t)(vo + rank);
      }
      if (ok)
        for (int c = 0; c < 3; ++c) out_faces[(base + written) * 3 + c] = idx[c];
      ++written;
    }
  }
  if (bad_table || written != want) atomicOr(flag, AM_ISO_BAD_TABLE);
}

}  // namespace

extern "C" int am_iso_classify(const am_iso_classify_args* a, void* stream) {
  AM_CHECK(a != nullptr, "am_iso_classify: null arguments");
  AM_TRY(check_grid("am_iso_classify", a->nx, a->ny, a->nz));
  AM_TRY(check_level("am_iso_classify", a->level));
  AM_CHECK(a->values && a->out_mask && a->out_count, "am_iso_classify: null pointer");
  dim3 blocks;
  AM_TRY(tile_blocks("am_iso_classify", a->nx, a->ny, a->nz, blocks));
  const grid_view g = {a->nx, a->ny, a->nz, a->level, a->inside_above != 0};
  hipLaunchKernelGGL(iso_classify_kernel, blocks, dim3(GRID_THREADS), 0, (hipStream_t)stream, g, a->values, a->out_mask, a->out_count);
  AM_HIP(hipGetLastError());
  return AM_OK;
}

extern "C" int am_iso_vertices(const am_iso_vertices_args* a, void* stream) {
  AM_CHECK(a != nullptr, "am_iso_vertices: null arguments");
  AM_TRY(check_grid("am_iso_vertices", a->nx, a->ny, a->nz));
  AM_TRY(check_level("am_iso_vertices", a->level));
  AM_TRY(check_count("am_iso_vertices", "vertices", a->n_vertices));
  AM_CHECK(a->values && a->mask && a->vertex_offset && a->out_vertices && a->out_flag, "am_iso_vertices: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const grid_view g = {a->nx, a->ny, a->nz, a->level, 1};
  AM_HIP(hipMemsetAsync(a->out_flag, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(iso_vertices_kernel, dim3(grid_blocks(a->nx * a->ny * a->nz)), dim3(GRID_THREADS), 0, st, g, a->values, a->mask,
                     a->vertex_offset, a->n_vertices, a->origin[0], a->origin[1], a->origin[2], a->spacing[0], a->spacing[1],
                     a->spacing[2], a->out_vertices, a->out_flag);
  AM_HIP(hipGetLastError());
  return AM_OK;
}

extern "C" int am_iso_triangles(const am_iso_triangles_args* a, void* stream) {
  AM_CHECK(a != nullptr, "am_iso_triangles: null arguments");
  AM_TRY(check_grid("am_iso_triangles", a->nx, a->ny, a->nz));
  AM_TRY(check_level("am_iso_triangles", a->level));
  AM_TRY(check_count("am_iso_triangles", "vertices", a->n_vertices));
  AM_TRY(check_count("am_iso_triangles", "triangles", a->n_triangles));
  AM_CHECK(a->values && a->mask && a->count && a->vertex_offset && a->tri_offset && a->out_faces && a->out_flag,
           "am_iso_triangles: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const grid_view g = {a->nx, a->ny, a->nz, a->level, a->inside_above != 0};
  AM_HIP(hipMemsetAsync(a->out_flag, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(iso_triangles_kernel, dim3(grid_blocks(a->nx * a->ny * a->nz)), dim3(GRID_THREADS), 0, st, g, a->values, a->mask,
                     a->count, a->vertex_offset, a->tri_offset, a->n_vertices, a->n_triangles, a->out_faces, a->out_flag);
  AM_HIP(hipGetLastError());
  return AM_OK;
}
