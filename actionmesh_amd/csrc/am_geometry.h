// What the fp64 mesh kernels share (am_mesh.hip, am_decimate.hip): the vector arithmetic whose association order is part of the
// bit-exact contract of include/actionmesh_amd.h, the validated reads of a face and of a vertex's corners, the size limit and the
// launch arithmetic.  Everything sits in the unnamed namespace, next to the kernels of the source that includes it.
#pragma once
#include "am_common.h"

#pragma clang fp contract(off)      // the helpers below too, whatever flags the file is built with

namespace {

constexpr int MESH_THREADS = 256;                               // every kernel: one thread per item, blocks of 256
constexpr int64_t MESH_MAX = (((int64_t)1 << 31) - 1) / 3;      // 3 * n fits an int32 corner id / element offset of one frame

unsigned mesh_blocks(int64_t n) { return (unsigned)((n + MESH_THREADS - 1) / MESH_THREADS); }

// the counts every entry point checks first, in its own name; am_vertex_normals alone takes a mesh without faces (min_faces 0)
int check_mesh(const char* who, int64_t n_vertices, int64_t n_faces, int min_faces = 1) {
  AM_CHECK(n_vertices >= 1 && n_vertices <= MESH_MAX, "%s: %lld vertices outside 1 .. (2^31 - 1) / 3", who, (long long)n_vertices);
  AM_CHECK(n_faces >= min_faces && n_faces <= MESH_MAX, "%s: %lld faces outside %d .. (2^31 - 1) / 3", who, (long long)n_faces, min_faces);
  return AM_OK;
}

struct vec3 {
  double x, y, z;
};

__device__ __forceinline__ vec3 sub3(vec3 a, vec3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot3(vec3 a, vec3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ double norm3(vec3 a) { return sqrt(dot3(a, a)); }
__device__ __forceinline__ vec3 div3(vec3 a, double s) { return {a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ vec3 cross3(vec3 a, vec3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ bool in_range(int i, int64_t n) { return i >= 0 && (int64_t)i < n; }

// vertex v of fp64 positions
__device__ __forceinline__ vec3 load3(const double* p, int v) {
  const int64_t o = (int64_t)v * 3;
  return {p[o], p[o + 1], p[o + 2]};
}
// element i, and vertex v of the frame that starts at element `base`, of fp32 (widened: exact) or fp64 storage
__device__ __forceinline__ double mesh_load(const void* p, int64_t i, int f64) {
  return f64 ? reinterpret_cast<const double*>(p)[i] : (double)reinterpret_cast<const float*>(p)[i];
}
__device__ __forceinline__ vec3 mesh_vertex(const void* verts, int64_t base, int v, int f64) {
  const int64_t o = base + (int64_t)v * 3;
  return {mesh_load(verts, o, f64), mesh_load(verts, o + 1, f64), mesh_load(verts, o + 2, f64)};
}

// the three vertex indices of a face, `face` pointing at the first of them; false, with AM_MESH_BAD_FACE raised, when one of them
// is outside [0, n_vertices)
__device__ __forceinline__ bool face_indices(const int32_t* face, int64_t n_vertices, int32_t* flag, int& i0, int& i1, int& i2) {
  i0 = face[0];
  i1 = face[1];
  i2 = face[2];
  if (in_range(i0, n_vertices) && in_range(i1, n_vertices) && in_range(i2, n_vertices)) return true;
  atomicOr(flag, AM_MESH_BAD_FACE);
  return false;
}

// what every kernel knows of the mesh (the edge tables: the decimator's)
struct mesh_view {
  int64_t n_vertices, n_faces, n_edges;
  const int32_t* faces;
  const int32_t* offsets;
  const int32_t* corners;
  const int32_t* edges;
  const int32_t* he2e;
  int32_t* flag;
};

// the validated corner range of vertex v (v already inside [0, n_vertices)); an invalid one is empty and raises the flag
__device__ __forceinline__ bool csr_range(const mesh_view& m, int v, int& begin, int& end) {
  begin = m.offsets[v];
  end = m.offsets[v + 1];
  if (begin < 0 || end < begin || (int64_t)end > 3 * m.n_faces) {
    atomicOr(m.flag, AM_MESH_BAD_CSR);
    begin = end = 0;
    return false;
  }
  return true;
}

// corner j of the range of vertex v: the corner id, or -1 (flag raised) when it is outside [0, 3 n_faces) or names another vertex
__device__ __forceinline__ int corner_at(const mesh_view& m, int j, int v) {
  const int c = m.corners[j];
  if (c < 0 || (int64_t)c >= 3 * m.n_faces || m.faces[c] != v) {
    atomicOr(m.flag, AM_MESH_BAD_CSR);
    return -1;
  }
  return c;
}

// the other two vertices of the face of corner c, in face order behind the corner; false (flag raised) when one is out of range
__device__ __forceinline__ bool corner_others(const mesh_view& m, int c, int& w1, int& w2) {
  const int f3 = c - c % 3, k = c % 3;
  w1 = m.faces[f3 + (k + 1) % 3];
  w2 = m.faces[f3 + (k + 2) % 3];
  if (!in_range(w1, m.n_vertices) || !in_range(w2, m.n_vertices)) {
    atomicOr(m.flag, AM_MESH_BAD_FACE);
    return false;
  }
  return true;
}

}  // namespace
