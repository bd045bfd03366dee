// Iso-surface extraction, the second method: dual marching cubes on a regular grid with a manifold rule (actionmesh_amd/isosurface.py,
// method="dual").  One vertex per patch of every active cell, one quad per crossing grid edge: about a third of the triangles of
// the marching tetrahedra of am_isosurface.hip.  The contract is include/actionmesh_amd.h's; the interpolation and the centroids are
// fp64, every operation rounded on its own (the file is built with -ffp-contract=off), so codes, counts, vertices and faces are
// compared bit for bit with a numpy restatement that derives the tables below from the header's rule.
//
//   am_dmc_cells       one block per 8 x 8 x 64 tile of points (am_grid.h's tile_walk): per cell its configuration and its double faces
//   am_dmc_classify    one thread per point: the cell's code (configuration + flip bit) from its own and its six neighbours' double
//                      faces, its number of patches, and the mask of the axis edges from the point that emit a quad
//   am_dmc_vertices    one thread per point: an active cell writes the centroids of its patches at vertex_offset[p] + patch
//   am_dmc_triangles   one thread per point: an emitting edge writes its two triangles at tri_offset[p] + 2 * rank of the edge
// The first two are separate kernels: the flip needs the neighbours' results on BOTH sides of every axis, which a fused kernel would
// recompute from a two-sided halo of values.  No atomics but the OR into the flag word, no hash table: the order of vertices and
// faces is fixed by the two prefix sums the caller makes.  No offset, code or index read from memory is used as an address before
// it has been compared with its bound.
// From am_grid.h, shared with am_isosurface.hip: the grid and point_state, the tile walk, the index arithmetic of a point and of a
// cell's corners, the crossing interpolation, the launch arithmetic and the host checks.  From am_geometry.h: vec3 and mesh_vertex.
#include "am_geometry.h"
#include "am_grid.h"

namespace {

constexpr uint32_t NO_PATCH = 15u;

// [flipped][configuration]: nibble e = the patch of cell edge e (15: the edge does not cross), nibble 12 = the number of patches.
// Row 1 differs from row 0 on the 36 configurations with a double face: that face cuts off its outside corners there.
__device__ const uint64_t DMC_PATCH[2][256] = {
    {
     0x0ffffffffffffull, 0x1fffffffff000ull, 0x1fffffff00ff0ull, 0x1fffffff0000full, 0x1fffff00fff0full, 0x1fffff00ff0f0ull,
     0x2fffff1100f10ull, 0x1fffff00000ffull, 0x1ffff0f0f0fffull, 0x2ffff1f1f1000ull, 0x1ffff0f00fff0ull, 0x1ffff0f00f00full,
     0x1ffff00ff0f0full, 0x1ffff00ff00f0ull, 0x1ffff00f0ff00ull, 0x1ffff00f0f0ffull, 0x1ff00fffff0ffull, 0x1ff00ffffff00ull,
     0x2ff11fff001f0ull, 0x1ff00fff00f0full, 0x2ff11f00ff10full, 0x1ff00f00ffff0ull, 0x3ff22f1100210ull, 0x1ff00f0000fffull,
     0x2ff001f1f10ffull, 0x2ff001f1f1f00ull, 0x2ff110f00f1f0ull, 0x1ff000f00ff0full, 0x2ff1100ff010full, 0x1ff0000ff0ff0ull,
     0x2ff1100f0f100ull, 0x1ff0000f0ffffull, 0x1f0f0fff0ffffull, 0x2f1f1fff1f000ull, 0x1f0f0ffff0ff0ull, 0x1f0f0ffff000full,
     0x2f1f1f001ff0full, 0x2f1f1f001f0f0ull, 0x2f0f0f11f0f10ull, 0x1f0f0f00f00ffull, 0x2f1f10f010fffull, 0x3f2f21f121000ull,
     0x1f0f00f0ffff0ull, 0x1f0f00f0ff00full, 0x2f1f100f10f0full, 0x2f1f100f100f0ull, 0x1f0f000ffff00ull, 0x1f0f000fff0ffull,
     0x1f00ffff0f0ffull, 0x1f00ffff0ff00ull, 0x1f00fffff00f0ull, 0x1f00fffff0f0full, 0x2f11ff001f10full, 0x1f00ff000fff0ull,
     0x2f00ff11f0010ull, 0x1f00ff00f0fffull, 0x2f00f1f1010ffull, 0x2f00f1f101f00ull, 0x1f00f0f0ff0f0ull, 0x1f00f0f0fff0full,
     0x2f11f00f1010full, 0x1f00f00f00ff0ull, 0x1f00f00fff000ull, 0x1f00f00ffffffull, 0x10f0ff0ffffffull, 0x21f1ff1fff000ull,
     0x21f1ff1f00ff0ull, 0x21f1ff1f0000full, 0x10f0fff0fff0full, 0x10f0fff0ff0f0ull, 0x21f1fff100f10ull, 0x10f0fff0000ffull,
     0x21f1f010f0fffull, 0x32f2f121f1000ull, 0x21f1f0100fff0ull, 0x21f1f0100f00full, 0x10f0f0fff0f0full, 0x10f0f0fff00f0ull,
     0x10f0f0ff0ff00ull, 0x10f0f0ff0f0ffull, 0x10ff0f0fff0ffull, 0x10ff0f0ffff00ull, 0x21ff1f1f001f0ull, 0x10ff0f0f00f0full,
     0x10ff0ff0ff00full, 0x10ff0ff0ffff0ull, 0x21ff1ff100110ull, 0x10ff0ff000fffull, 0x20ff0101f10ffull, 0x20ff0101f1f00ull,
     0x21ff10100f1f0ull, 0x10ff00000ff0full, 0x10ff00fff000full, 0x10ff00fff0ff0ull, 0x10ff00ff0f000ull, 0x10ff00ff0ffffull,
     0x21010f1f0ffffull, 0x32121f2f1f000ull, 0x21010f1ff0ff0ull, 0x21010f1ff000full, 0x20101ff01ff0full, 0x20101ff01f0f0ull,
     0x21010ff1f0f10ull, 0x10000ff0f00ffull, 0x3212102010fffull, 0x4323213121000ull, 0x21010010ffff0ull, 0x21010010ff00full,
     0x201010ff10f0full, 0x201010ff100f0ull, 0x100000fffff00ull, 0x100000ffff0ffull, 0x100fff0f0f0ffull, 0x100fff0f0ff00ull,
     0x100fff0ff00f0ull, 0x100fff0ff0f0full, 0x100ffff00f00full, 0x100ffff00fff0ull, 0x100ffff0f0000ull, 0x100ffff0f0fffull,
     0x200ff101010ffull, 0x200ff10101f00ull, 0x100ff000ff0f0ull, 0x100ff000fff0full, 0x100ff0ff0000full, 0x100ff0ff00ff0ull,
     0x211ff1ffff000ull, 0x100ff0fffffffull, 0x100ff0fffffffull, 0x211ff1ffff000ull, 0x211ff1ff00ff0ull, 0x211ff1ff0000full,
     0x211ff100fff0full, 0x211ff100ff0f0ull, 0x322ff21100f10ull, 0x211ff100000ffull, 0x100ffff0f0fffull, 0x211ffff1f1000ull,
     0x100ffff00fff0ull, 0x100ffff00f00full, 0x100fff0ff0f0full, 0x100fff0ff00f0ull, 0x100fff0f0ff00ull, 0x100fff0f0f0ffull,
     0x211001ffff0ffull, 0x211001fffff00ull, 0x322112ff001f0ull, 0x211001ff00f0full, 0x32211200ff10full, 0x21100100ffff0ull,
     0x4332231100210ull, 0x2110010000fffull, 0x21100ff1f10ffull, 0x21100ff1f1f00ull, 0x20011ff00f1f0ull, 0x10000ff00ff0full,
     0x20011f0ff010full, 0x10000f0ff0ff0ull, 0x20011f0f0f100ull, 0x10000f0f0ffffull, 0x10ff00ff0ffffull, 0x21ff11ff1f000ull,
     0x10ff00fff0ff0ull, 0x10ff00fff000full, 0x21ff11001ff0full, 0x21ff11001f0f0ull, 0x20ff0011f0f10ull, 0x10ff0000f00ffull,
     0x10ff0ff000fffull, 0x21ff1ff111000ull, 0x10ff0ff0ffff0ull, 0x10ff0ff0ff00full, 0x10ff0f0f00f0full, 0x10ff0f0f000f0ull,
     0x10ff0f0ffff00ull, 0x10ff0f0fff0ffull, 0x10f0f0ff0f0ffull, 0x10f0f0ff0ff00ull, 0x10f0f0fff00f0ull, 0x10f0f0fff0f0full,
     0x21f1f1001f10full, 0x10f0f0000fff0ull, 0x20f0f011f0010ull, 0x10f0f000f0fffull, 0x10f0fff0000ffull, 0x10f0fff000f00ull,
     0x10f0fff0ff0f0ull, 0x10f0fff0fff0full, 0x10f0ff0f0000full, 0x21f1ff1f00ff0ull, 0x10f0ff0fff000ull, 0x10f0ff0ffffffull,
     0x1f00f00ffffffull, 0x2f11f11fff000ull, 0x2f11f11f00ff0ull, 0x2f11f11f0000full, 0x1f00f0f0fff0full, 0x1f00f0f0ff0f0ull,
     0x2f11f1f100f10ull, 0x1f00f0f0000ffull, 0x1f00ff00f0fffull, 0x2f11ff11f1000ull, 0x1f00ff000fff0ull, 0x1f00ff000f00full,
     0x1f00fffff0f0full, 0x1f00fffff00f0ull, 0x1f00ffff0ff00ull, 0x1f00ffff0f0ffull, 0x1f0f000fff0ffull, 0x1f0f000ffff00ull,
     0x2f1f111f001f0ull, 0x1f0f000f00f0full, 0x1f0f00f0ff00full, 0x1f0f00f0ffff0ull, 0x2f1f11f100110ull, 0x1f0f00f000fffull,
     0x1f0f0f00f00ffull, 0x1f0f0f00f0f00ull, 0x1f0f0f000f0f0ull, 0x2f1f1f001ff0full, 0x1f0f0ffff000full, 0x1f0f0ffff0ff0ull,
     0x1f0f0fff0f000ull, 0x1f0f0fff0ffffull, 0x1ff0000f0ffffull, 0x2ff1111f1f000ull, 0x1ff0000ff0ff0ull, 0x1ff0000ff000full,
     0x1ff000f00ff0full, 0x1ff000f00f0f0ull, 0x1ff000f0f0f00ull, 0x2ff001f1f10ffull, 0x1ff00f0000fffull, 0x2ff11f1111000ull,
     0x1ff00f00ffff0ull, 0x1ff00f00ff00full, 0x1ff00fff00f0full, 0x1ff00fff000f0ull, 0x1ff00ffffff00ull, 0x1ff00fffff0ffull,
     0x1ffff00f0f0ffull, 0x1ffff00f0ff00ull, 0x1ffff00ff00f0ull, 0x1ffff00ff0f0full, 0x1ffff0f00f00full, 0x1ffff0f00fff0ull,
     0x1ffff0f0f0000ull, 0x1ffff0f0f0fffull, 0x1fffff00000ffull, 0x1fffff0000f00ull, 0x1fffff00ff0f0ull, 0x1fffff00fff0full,
     0x1fffffff0000full, 0x1fffffff00ff0ull, 0x1fffffffff000ull, 0x0ffffffffffffull,
    },
    {
     0x0ffffffffffffull, 0x1fffffffff000ull, 0x1fffffff00ff0ull, 0x1fffffff0000full, 0x1fffff00fff0full, 0x1fffff00ff0f0ull,
     0x2fffff1100f10ull, 0x1fffff00000ffull, 0x1ffff0f0f0fffull, 0x2ffff1f1f1000ull, 0x1ffff0f00fff0ull, 0x1ffff0f00f00full,
     0x1ffff00ff0f0full, 0x1ffff00ff00f0ull, 0x1ffff00f0ff00ull, 0x1ffff00f0f0ffull, 0x1ff00fffff0ffull, 0x1ff00ffffff00ull,
     0x2ff11fff001f0ull, 0x1ff00fff00f0full, 0x2ff11f00ff10full, 0x1ff00f00ffff0ull, 0x3ff22f1100210ull, 0x1ff00f0000fffull,
     0x2ff001f1f10ffull, 0x2ff001f1f1f00ull, 0x2ff110f00f1f0ull, 0x1ff000f00ff0full, 0x2ff1100ff010full, 0x1ff0000ff0ff0ull,
     0x2ff1100f0f100ull, 0x1ff0000f0ffffull, 0x1f0f0fff0ffffull, 0x2f1f1fff1f000ull, 0x1f0f0ffff0ff0ull, 0x1f0f0ffff000full,
     0x2f1f1f001ff0full, 0x2f1f1f001f0f0ull, 0x2f0f0f11f0f10ull, 0x1f0f0f00f00ffull, 0x2f1f10f010fffull, 0x3f2f21f121000ull,
     0x1f0f00f0ffff0ull, 0x1f0f00f0ff00full, 0x2f1f100f10f0full, 0x2f1f100f100f0ull, 0x1f0f000ffff00ull, 0x1f0f000fff0ffull,
     0x1f00ffff0f0ffull, 0x1f00ffff0ff00ull, 0x1f00fffff00f0ull, 0x1f00fffff0f0full, 0x2f11ff001f10full, 0x1f00ff000fff0ull,
     0x2f00ff11f0010ull, 0x1f00ff00f0fffull, 0x2f00f1f1010ffull, 0x2f00f1f101f00ull, 0x1f00f0f0ff0f0ull, 0x1f00f0f0fff0full,
     0x2f11f00f1010full, 0x2f11f11f00ff0ull, 0x2f11f11fff000ull, 0x1f00f00ffffffull, 0x10f0ff0ffffffull, 0x21f1ff1fff000ull,
     0x21f1ff1f00ff0ull, 0x21f1ff1f0000full, 0x10f0fff0fff0full, 0x10f0fff0ff0f0ull, 0x21f1fff100f10ull, 0x10f0fff0000ffull,
     0x21f1f010f0fffull, 0x32f2f121f1000ull, 0x21f1f0100fff0ull, 0x21f1f0100f00full, 0x10f0f0fff0f0full, 0x10f0f0fff00f0ull,
     0x10f0f0ff0ff00ull, 0x10f0f0ff0f0ffull, 0x10ff0f0fff0ffull, 0x10ff0f0ffff00ull, 0x21ff1f1f001f0ull, 0x10ff0f0f00f0full,
     0x10ff0ff0ff00full, 0x10ff0ff0ffff0ull, 0x21ff1ff100110ull, 0x10ff0ff000fffull, 0x20ff0101f10ffull, 0x20ff0101f1f00ull,
     0x21ff10100f1f0ull, 0x21ff11001ff0full, 0x10ff00fff000full, 0x10ff00fff0ff0ull, 0x21ff11ff1f000ull, 0x10ff00ff0ffffull,
     0x21010f1f0ffffull, 0x32121f2f1f000ull, 0x21010f1ff0ff0ull, 0x21010f1ff000full, 0x20101ff01ff0full, 0x20101ff01f0f0ull,
     0x21010ff1f0f10ull, 0x21100ff1f10ffull, 0x3212102010fffull, 0x4323213121000ull, 0x21010010ffff0ull, 0x21010010ff00full,
     0x201010ff10f0full, 0x201010ff100f0ull, 0x211001fffff00ull, 0x211001ffff0ffull, 0x100fff0f0f0ffull, 0x100fff0f0ff00ull,
     0x100fff0ff00f0ull, 0x100fff0ff0f0full, 0x100ffff00f00full, 0x100ffff00fff0ull, 0x211ffff1f1000ull, 0x100ffff0f0fffull,
     0x200ff101010ffull, 0x200ff10101f00ull, 0x211ff100ff0f0ull, 0x211ff100fff0full, 0x211ff1ff0000full, 0x211ff1ff00ff0ull,
     0x211ff1ffff000ull, 0x100ff0fffffffull, 0x100ff0fffffffull, 0x211ff1ffff000ull, 0x211ff1ff00ff0ull, 0x211ff1ff0000full,
     0x211ff100fff0full, 0x211ff100ff0f0ull, 0x322ff21100f10ull, 0x211ff100000ffull, 0x100ffff0f0fffull, 0x211ffff1f1000ull,
     0x100ffff00fff0ull, 0x100ffff00f00full, 0x100fff0ff0f0full, 0x100fff0ff00f0ull, 0x100fff0f0ff00ull, 0x100fff0f0f0ffull,
     0x211001ffff0ffull, 0x211001fffff00ull, 0x322112ff001f0ull, 0x211001ff00f0full, 0x32211200ff10full, 0x21100100ffff0ull,
     0x4332231100210ull, 0x2110010000fffull, 0x21100ff1f10ffull, 0x21100ff1f1f00ull, 0x20011ff00f1f0ull, 0x20101ff01ff0full,
     0x20011f0ff010full, 0x21010f1ff0ff0ull, 0x20011f0f0f100ull, 0x21010f1f0ffffull, 0x10ff00ff0ffffull, 0x21ff11ff1f000ull,
     0x10ff00fff0ff0ull, 0x10ff00fff000full, 0x21ff11001ff0full, 0x21ff11001f0f0ull, 0x20ff0011f0f10ull, 0x20ff0101f10ffull,
     0x10ff0ff000fffull, 0x21ff1ff111000ull, 0x10ff0ff0ffff0ull, 0x10ff0ff0ff00full, 0x10ff0f0f00f0full, 0x21ff1f1f001f0ull,
     0x10ff0f0ffff00ull, 0x10ff0f0fff0ffull, 0x10f0f0ff0f0ffull, 0x10f0f0ff0ff00ull, 0x10f0f0fff00f0ull, 0x10f0f0fff0f0full,
     0x21f1f1001f10full, 0x21f1f0100fff0ull, 0x20f0f011f0010ull, 0x21f1f010f0fffull, 0x10f0fff0000ffull, 0x21f1fff100f10ull,
     0x10f0fff0ff0f0ull, 0x10f0fff0fff0full, 0x21f1ff1f0000full, 0x21f1ff1f00ff0ull, 0x21f1ff1fff000ull, 0x10f0ff0ffffffull,
     0x1f00f00ffffffull, 0x2f11f11fff000ull, 0x2f11f11f00ff0ull, 0x2f11f11f0000full, 0x1f00f0f0fff0full, 0x1f00f0f0ff0f0ull,
     0x2f11f1f100f10ull, 0x2f00f1f1010ffull, 0x1f00ff00f0fffull, 0x2f11ff11f1000ull, 0x1f00ff000fff0ull, 0x2f11ff001f10full,
     0x1f00fffff0f0full, 0x1f00fffff00f0ull, 0x1f00ffff0ff00ull, 0x1f00ffff0f0ffull, 0x1f0f000fff0ffull, 0x1f0f000ffff00ull,
     0x2f1f111f001f0ull, 0x2f1f100f10f0full, 0x1f0f00f0ff00full, 0x1f0f00f0ffff0ull, 0x2f1f11f100110ull, 0x2f1f10f010fffull,
     0x1f0f0f00f00ffull, 0x2f0f0f11f0f10ull, 0x2f1f1f001f0f0ull, 0x2f1f1f001ff0full, 0x1f0f0ffff000full, 0x1f0f0ffff0ff0ull,
     0x2f1f1fff1f000ull, 0x1f0f0fff0ffffull, 0x1ff0000f0ffffull, 0x2ff1111f1f000ull, 0x1ff0000ff0ff0ull, 0x2ff1100ff010full,
     0x1ff000f00ff0full, 0x2ff110f00f1f0ull, 0x2ff001f1f1f00ull, 0x2ff001f1f10ffull, 0x1ff00f0000fffull, 0x2ff11f1111000ull,
     0x1ff00f00ffff0ull, 0x2ff11f00ff10full, 0x1ff00fff00f0full, 0x2ff11fff001f0ull, 0x1ff00ffffff00ull, 0x1ff00fffff0ffull,
     0x1ffff00f0f0ffull, 0x1ffff00f0ff00ull, 0x1ffff00ff00f0ull, 0x1ffff00ff0f0full, 0x1ffff0f00f00full, 0x1ffff0f00fff0ull,
     0x2ffff1f1f1000ull, 0x1ffff0f0f0fffull, 0x1fffff00000ffull, 0x2fffff1100f10ull, 0x1fffff00ff0f0ull, 0x1fffff00fff0full,
     0x1fffffff0000full, 0x1fffffff00ff0ull, 0x1fffffffff000ull, 0x0ffffffffffffull,
    },
};
// the 6-bit mask of a configuration's double faces, face 2 axis + side (at most one bit)
__device__ const uint8_t DMC_DOUBLE[256] = {
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 32, 16, 0,
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 8, 0, 0, 4, 0,
    0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 2, 2, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 8, 8, 32, 32, 0, 0,
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 2, 0, 2,
    0, 0, 0, 0, 0, 0, 0, 8, 0, 0, 0, 0, 0, 4, 0, 0, 0, 0, 0, 0, 0, 8, 0, 8, 0, 1, 0, 0, 16, 0, 16, 0,
    0, 0, 0, 0, 0, 0, 0, 32, 0, 0, 0, 16, 0, 0, 0, 0, 0, 0, 0, 32, 0, 0, 0, 32, 0, 1, 4, 0, 0, 0, 4, 0,
    0, 0, 0, 16, 0, 4, 1, 0, 0, 0, 0, 16, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0,
};
// [corner a][axis]: the id of the cell edge from corner a along the axis (255: a is the far end)
__device__ const uint8_t DMC_EDGE_ID[8][3] = {{2, 1, 0}, {4, 3, 255}, {6, 255, 5}, {7, 255, 255}, {255, 9, 8}, {255, 10, 255},
                                              {255, 255, 11}, {255, 255, 255}};
// the two corners of cell edge e, a < b, in ascending (a, b)
__device__ const uint8_t DMC_EDGE[12][2] = {{0, 1}, {0, 2}, {0, 4}, {1, 3}, {1, 5}, {2, 3}, {2, 6}, {3, 7}, {4, 5}, {4, 6}, {5, 7}, {6, 7}};

// the configuration of a cell from the states of its corners: 0 unless the cell is ACTIVE
__device__ __forceinline__ uint32_t cell_config(const uint32_t (&s)[8]) {
  uint32_t finite = 1u, cfg = 0u;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    finite &= s[m];
    cfg |= (s[m] >> 1) << m;
  }
  return (finite & 1u) && cfg != 255u ? cfg : 0u;
}

// a cell code as am_dmc_classify writes it: configuration 1 .. 254, + 256 only where the configuration has a double face
__device__ __forceinline__ bool code_valid(uint32_t code) {
  const uint32_t cfg = code & 255u;
  return code <= 511u && cfg != 0u && cfg != 255u && (code < 256u || DMC_DOUBLE[cfg] != 0);
}

__global__ __launch_bounds__(GRID_THREADS) void dmc_cells_kernel(grid_view g, const float* __restrict__ values,
                                                                 uint8_t* __restrict__ out_config, uint8_t* __restrict__ out_double) {
  tile_walk(g, values, [=](int64_t p, cell_states c) {
    const uint32_t cfg = cell_config(c.s);
    out_config[p] = (uint8_t)cfg;
    out_double[p] = DMC_DOUBLE[cfg];
  });
}

__global__ __launch_bounds__(GRID_THREADS) void dmc_classify_kernel(int64_t nx, int64_t ny, int64_t nz, const uint8_t* __restrict__ config,
                                                                    const uint8_t* __restrict__ dbl, int16_t* __restrict__ out_code,
                                                                    uint8_t* __restrict__ out_count, uint8_t* __restrict__ out_mask) {
  const int64_t p = (int64_t)blockIdx.x * GRID_THREADS + threadIdx.x;
  if (p >= nx * ny * nz) return;
  const uint32_t cfg = config[p];
  uint32_t flip = 0u, mask = 0u;
  if (cfg != 0u) {
    const grid_point at = point_at(p, ny, nz);
    const grid_steps step = steps_of(ny, nz);
    const int64_t idx[3] = {at.i, at.j, at.k}, n[3] = {nx, ny, nz};
    const uint32_t d = dbl[p];
    for (int axis = 0; axis < 3 && d != 0u; ++axis) {             // a face is flipped when it is double on both of its sides
      if ((d >> (2 * axis) & 1u) && idx[axis] >= 1 && (dbl[p - step.s[axis]] >> (2 * axis + 1) & 1u)) flip = 1u;
      if ((d >> (2 * axis + 1) & 1u) && idx[axis] + 1 < n[axis] && (dbl[p + step.s[axis]] >> (2 * axis) & 1u)) flip = 1u;
    }
    for (int axis = 0; axis < 3; ++axis) {
      const int u = (axis + 1) % 3, v = (axis + 2) % 3;
      if (idx[u] < 1 || idx[v] < 1) continue;                     // one of the four cells around the edge does not exist
      if (((cfg ^ (cfg >> (4 >> axis))) & 1u) == 0u) continue;    // corner 000 and the corner along the axis on one side
      if (config[p - step.s[u]] != 0 && config[p - step.s[u] - step.s[v]] != 0 && config[p - step.s[v]] != 0) mask |= 1u << axis;
    }
  }
  out_code[p] = (int16_t)(cfg | flip << 8);
  out_count[p] = (uint8_t)(DMC_PATCH[flip][cfg] >> 48 & 15u);
  out_mask[p] = (uint8_t)mask;
}

__global__ __launch_bounds__(GRID_THREADS) void dmc_vertices_kernel(grid_view g, const float* __restrict__ values,
                                                                    const int16_t* __restrict__ code,
                                                                    const int64_t* __restrict__ vertex_offset, int64_t n_vertices,
                                                                    double ox, double oy, double oz, double sx, double sy, double sz,
                                                                    float* __restrict__ out_vertices, int32_t* flag) {
#pragma clang fp contract(off)
  const int64_t p = (int64_t)blockIdx.x * GRID_THREADS + threadIdx.x;
  if (p >= g.nx * g.ny * g.nz) return;
  const uint32_t c = (uint16_t)code[p];
  if (c == 0u) return;
  const grid_point at = point_at(p, g.ny, g.nz);
  if (!code_valid(c) || at.i + 1 >= g.nx || at.j + 1 >= g.ny || at.k + 1 >= g.nz) {   // no such code, or a code where no cell starts
    atomicOr(flag, AM_DMC_BAD_CODE);
    return;
  }
  const grid_steps step = steps_of(g.ny, g.nz);
  double value[8];
  uint32_t s[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const float v = values[cell_corner(p, step, m)];
    value[m] = (double)v;
    s[m] = point_state(v, g.level, g.inside_above);
  }
  if (cell_config(s) != (c & 255u)) {                             // the code is not the one these values give
    atomicOr(flag, AM_DMC_BAD_CODE);
    return;
  }
  const uint64_t table = DMC_PATCH[c >> 8][c & 255u];
  const int64_t patches = (int64_t)(table >> 48 & 15u);
  const int64_t base = vertex_offset[p];
  if (base < 0 || base > n_vertices - patches) {
    atomicOr(flag, AM_DMC_BAD_VERTEX_OFFSET);
    return;
  }
  const double org[3] = {ox, oy, oz}, sp[3] = {sx, sy, sz};
  const int64_t idx[3] = {at.i, at.j, at.k};
  for (int64_t q = 0; q < patches; ++q) {
    double sum[3] = {0.0, 0.0, 0.0};
    int number = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) {                                // ascending edge id: the order of the sum
      if ((int64_t)(table >> (4 * e) & 15u) != q) continue;
      const int a = DMC_EDGE[e][0], b = DMC_EDGE[e][1];
      for (int x = 0; x < 3; ++x) {
        const double pa = org[x] + (double)(idx[x] + (a >> (2 - x) & 1)) * sp[x];
        const double pb = org[x] + (double)(idx[x] + (b >> (2 - x) & 1)) * sp[x];
        sum[x] = sum[x] + crossing(g.level, value[a], value[b], pa, pb);
      }
      ++number;
    }
    for (int x = 0; x < 3; ++x) out_vertices[(base + q) * 3 + x] = (float)(sum[x] / (double)number);
  }
}

__global__ __launch_bounds__(GRID_THREADS) void dmc_triangles_kernel(int64_t nx, int64_t ny, int64_t nz, const int16_t* __restrict__ code,
                                                                     const uint8_t* __restrict__ edge_mask,
                                                                     const int64_t* __restrict__ vertex_offset,
                                                                     const int64_t* __restrict__ tri_offset,
                                                                     const float* __restrict__ vertices, int64_t n_vertices,
                                                                     int64_t n_triangles, int32_t* __restrict__ out_faces, int32_t* flag) {
#pragma clang fp contract(off)
  const int64_t p = (int64_t)blockIdx.x * GRID_THREADS + threadIdx.x;
  if (p >= nx * ny * nz) return;
  const uint32_t mk = edge_mask[p];
  if (mk == 0u) return;
  const grid_point at = point_at(p, ny, nz);
  const grid_steps step = steps_of(ny, nz);
  const int64_t idx[3] = {at.i, at.j, at.k};
  if (mk > 7u || idx[0] + 1 >= nx || idx[1] + 1 >= ny || idx[2] + 1 >= nz) {   // no such mask, or a mask where no cell starts
    atomicOr(flag, AM_DMC_BAD_CODE);
    return;
  }
  const int64_t base = tri_offset[p];
  if (base < 0 || base > n_triangles - 2 * (int64_t)__popc(mk)) {
    atomicOr(flag, AM_DMC_BAD_TRI_OFFSET);
    return;
  }
  int64_t rank = 0;
  for (int axis = 0; axis < 3; ++axis) {
    if (!(mk >> axis & 1u)) continue;
    const int64_t row = base + 2 * rank++;
    const int u = (axis + 1) % 3, v = (axis + 2) % 3;
    if (idx[u] < 1 || idx[v] < 1) {                               // one of the four cells around the edge does not exist
      atomicOr(flag, AM_DMC_BAD_CODE);
      continue;
    }
    int32_t q[4];
    bool ok = true, lower_inside = false;
    for (int r = 0; r < 4; ++r) {                                 // around the edge: p, p - e_u, p - e_u - e_v, p - e_v
      const int du = r == 1 || r == 2, dv = r >= 2;
      const int64_t cell = p - du * step.s[u] - dv * step.s[v];
      const uint32_t c = (uint16_t)code[cell];
      if (!code_valid(c)) {
        atomicOr(flag, AM_DMC_BAD_CODE);
        ok = false;
        continue;
      }
      const int corner = du * (4 >> u) + dv * (4 >> v);           // the corner of that cell at p
      const uint32_t patch = (uint32_t)(DMC_PATCH[c >> 8][c & 255u] >> (4 * DMC_EDGE_ID[corner][axis]) & 15u);
      if (patch == NO_PATCH) {                                    // the edge does not cross in that cell's configuration
        atomicOr(flag, AM_DMC_BAD_CODE);
        ok = false;
        continue;
      }
      const int64_t vo = vertex_offset[cell];
      if (vo < 0 || vo >= n_vertices - (int64_t)patch) {
        atomicOr(flag, AM_DMC_BAD_VERTEX_OFFSET);
        ok = false;
        continue;
      }
      q[r] = (int32_t)(vo + patch);
      if (r == 0) lower_inside = (c & 1u) != 0u;
    }
    if (!ok) continue;
    if (!lower_inside) {                                          // the normal points from the inside to the outside
      const int32_t t = q[1];
      q[1] = q[3];
      q[3] = t;
    }
    vec3 pos[4];
    for (int r = 0; r < 4; ++r) pos[r] = mesh_vertex(vertices, 0, q[r], 0);
    const vec3 d02 = sub3(pos[0], pos[2]), d13 = sub3(pos[1], pos[3]);
    const bool second = dot3(d13, d13) < dot3(d02, d02);          // the shorter diagonal; a tie goes to first - third
    const int32_t tri[2][3] = {{q[0], q[1], second ? q[3] : q[2]}, {second ? q[1] : q[0], q[2], q[3]}};
    for (int t = 0; t < 2; ++t)
      for (int x = 0; x < 3; ++x) out_faces[(row + t) * 3 + x] = tri[t][x];
  }
}

}  // namespace

extern "C" int am_dmc_cells(const am_dmc_cells_args* a, void* stream) {
  AM_CHECK(a != nullptr, "am_dmc_cells: null arguments");
  AM_TRY(check_grid("am_dmc_cells", a->nx, a->ny, a->nz));
  AM_TRY(check_level("am_dmc_cells", a->level));
  AM_CHECK(a->values && a->out_config && a->out_double, "am_dmc_cells: null pointer");
  dim3 blocks;
  AM_TRY(tile_blocks("am_dmc_cells", a->nx, a->ny, a->nz, blocks));
  const grid_view g = {a->nx, a->ny, a->nz, a->level, a->inside_above != 0};
  hipLaunchKernelGGL(dmc_cells_kernel, blocks, dim3(GRID_THREADS), 0, (hipStream_t)stream, g, a->values, a->out_config, a->out_double);
  AM_HIP(hipGetLastError());
  return AM_OK;
}

extern "C" int am_dmc_classify(const am_dmc_classify_args* a, void* stream) {
  AM_CHECK(a != nullptr, "am_dmc_classify: null arguments");
  AM_TRY(check_grid("am_dmc_classify", a->nx, a->ny, a->nz));
  AM_CHECK(a->config && a->double_faces && a->out_code && a->out_count && a->out_edge_mask, "am_dmc_classify: null pointer");
  hipLaunchKernelGGL(dmc_classify_kernel, dim3(grid_blocks(a->nx * a->ny * a->nz)), dim3(GRID_THREADS), 0, (hipStream_t)stream, a->nx,
                     a->ny, a->nz, a->config, a->double_faces, a->out_code, a->out_count, a->out_edge_mask);
  AM_HIP(hipGetLastError());
  return AM_OK;
}

extern "C" int am_dmc_vertices(const am_dmc_vertices_args* a, void* stream) {
  AM_CHECK(a != nullptr, "am_dmc_vertices: null arguments");
  AM_TRY(check_grid("am_dmc_vertices", a->nx, a->ny, a->nz));
  AM_TRY(check_level("am_dmc_vertices", a->level));
  AM_TRY(check_count("am_dmc_vertices", "vertices", a->n_vertices));
  AM_CHECK(a->values && a->code && a->vertex_offset && a->out_vertices && a->out_flag, "am_dmc_vertices: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const grid_view g = {a->nx, a->ny, a->nz, a->level, a->inside_above != 0};
  AM_HIP(hipMemsetAsync(a->out_flag, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(dmc_vertices_kernel, dim3(grid_blocks(a->nx * a->ny * a->nz)), dim3(GRID_THREADS), 0, st, g, a->values, a->code,
                     a->vertex_offset, a->n_vertices, a->origin[0], a->origin[1], a->origin[2], a->spacing[0], a->spacing[1],
                     a->spacing[2], a->out_vertices, a->out_flag);
  AM_HIP(hipGetLastError());
  return AM_OK;
}

extern "C" int am_dmc_triangles(const am_dmc_triangles_args* a, void* stream) {
  AM_CHECK(a != nullptr, "am_dmc_triangles: null arguments");
  AM_TRY(check_grid("am_dmc_triangles", a->nx, a->ny, a->nz));
  AM_TRY(check_count("am_dmc_triangles", "vertices", a->n_vertices));
  AM_TRY(check_count("am_dmc_triangles", "triangles", a->n_triangles));
  AM_CHECK(a->code && a->edge_mask && a->vertex_offset && a->tri_offset && a->vertices && a->out_faces && a->out_flag,
           "am_dmc_triangles: null pointer");
  hipStream_t st = (hipStream_t)stream;
  AM_HIP(hipMemsetAsync(a->out_flag, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(dmc_triangles_kernel, dim3(grid_blocks(a->nx * a->ny * a->nz)), dim3(GRID_THREADS), 0, st, a->nx, a->ny, a->nz, a->code,
                     a->edge_mask, a->vertex_offset, a->tri_offset, a->vertices, a->n_vertices, a->n_triangles, a->out_faces, a->out_flag);
  AM_HIP(hipGetLastError());
  return AM_OK;
}
