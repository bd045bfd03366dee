// Anchor-mesh preparation: trimesh's angle-weighted vertex normals for the frames of an animated mesh (reference
// actionmesh/preprocessing/mesh_processor.py:85-101 through mesh.vertex_normals), face areas, and trimesh.sample.sample_surface with
// the caller's uniforms (mesh_processor.py:245-285).  The contract is include/actionmesh_amd.h's; all geometry is fp64, every
// operation rounded on its own (the file is built with -ffp-contract=off), so the sample points are compared bit for bit with a numpy
// restatement and the normals to two fp32 ulps.
//
//   am_vertex_normals, whatever the valence and n_frames (one memset, two launches):
//     face     one thread per (frame, face): validates the three indices, stages the unit face normal and the three corner angles
//              in the workspace as six doubles { nx, ny, nz, a0, a1, a2 }; a face with a bad index stages zeros and raises the flag
//     vertex   one thread per (frame, vertex): walks its corners in CSR order (validating offsets and corners: a corner must name
//              this vertex), sums angle * face normal in fp64 in that order, normalises, rounds to fp32, normalises again in fp32.
//              A gather: no floating-point atomics, so the bits do not depend on scheduling.
//   am_face_areas and am_surface_sample: one launch each, one thread per face / per sample.
// No index read from memory is ever used as an address before it has been compared with its bound.
#include "am_geometry.h"

namespace {

constexpr double MESH_PI = 3.14159265358979323846;

__device__ __forceinline__ double clip1(double x) { return x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x); }

// c = e1 x e2 and |c|; the unit normal is c / |c|, or zero when |c| <= AM_MESH_ZERO
__device__ __forceinline__ vec3 unit_normal(vec3 c, double len) {
  if (!(len > AM_MESH_ZERO)) return {0.0, 0.0, 0.0};
  return div3(c, len);
}

// grid (face blocks, n_frames)
__global__ __launch_bounds__(MESH_THREADS) void mesh_face_kernel(const void* __restrict__ verts, int f64, int64_t frame_stride,
                                                                 int64_t n_vertices, int64_t n_faces, const int32_t* __restrict__ faces,
                                                                 double* __restrict__ staged, double* __restrict__ out_face_normals,
                                                                 int32_t* __restrict__ flag) {
#pragma clang fp contract(off)
  const int64_t f = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (f >= n_faces) return;
  const int t = blockIdx.y;
  vec3 n = {0.0, 0.0, 0.0};
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  int i0, i1, i2;
  if (face_indices(faces + 3 * f, n_vertices, flag, i0, i1, i2)) {
    const int64_t base = (int64_t)t * frame_stride;
    const vec3 v0 = mesh_vertex(verts, base, i0, f64), v1 = mesh_vertex(verts, base, i1, f64), v2 = mesh_vertex(verts, base, i2, f64);
    const vec3 e1 = sub3(v1, v0), e2 = sub3(v2, v0), e3 = sub3(v2, v1);
    const vec3 c = cross3(e1, e2);
    const double len = norm3(c);
    n = unit_normal(c, len);
    if (len > AM_MESH_ZERO) {
      const vec3 u = div3(e1, norm3(e1)), v = div3(e2, norm3(e2)), w = div3(e3, norm3(e3));
      a0 = acos(clip1(dot3(u, v)));
      a1 = acos(clip1(-dot3(u, w)));
      a2 = (MESH_PI - a0) - a1;
    }
  }
  double* s = staged + ((int64_t)t * n_faces + f) * 6;
  s[0] = n.x;
  s[1] = n.y;
  s[2] = n.z;
  s[3] = a0;
  s[4] = a1;
  s[5] = a2;
  if (out_face_normals) {
    double* o = out_face_normals + ((int64_t)t * n_faces + f) * 3;
    o[0] = n.x;
    o[1] = n.y;
    o[2] = n.z;
  }
}

// grid (vertex blocks, n_frames)
__global__ __launch_bounds__(MESH_THREADS) void mesh_vertex_kernel(mesh_view m, const void* __restrict__ verts, int f64,
                                                                   int64_t frame_stride, const double* __restrict__ staged,
                                                                   float* __restrict__ out_features, float* __restrict__ out_normals) {
#pragma clang fp contract(off)
  const int64_t v = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v >= m.n_vertices) return;
  const int t = blockIdx.y;
  int begin, end;
  csr_range(m, (int)v, begin, end);
  const double* st = staged + (int64_t)t * m.n_faces * 6;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int j = begin; j < end; ++j) {
    const int c = corner_at(m, j, (int)v);
    if (c < 0) continue;
    const double* s = st + (int64_t)(c / 3) * 6;
    const double a = s[3 + c % 3];
    sx = sx + a * s[0];
    sy = sy + a * s[1];
    sz = sz + a * s[2];
  }
  const double len = sqrt((sx * sx + sy * sy) + sz * sz);
  float nx = 0.f, ny = 0.f, nz = 0.f;
  if (len > AM_MESH_ZERO) {
    nx = (float)(sx / len);
    ny = (float)(sy / len);
    nz = (float)(sz / len);
  }
  // the reference's second normalisation, torch.nn.functional.normalize in fp32: x / max(||x||, 1e-12)
  float l32 = sqrtf((nx * nx + ny * ny) + nz * nz);
  l32 = l32 > 1e-12f ? l32 : 1e-12f;
  nx = nx / l32;
  ny = ny / l32;
  nz = nz / l32;
  const int64_t row = (int64_t)t * m.n_vertices + v;
  if (out_features) {
    const int64_t src = (int64_t)t * frame_stride + v * 3;
    float* o = out_features + row * 6;
    o[0] = (float)mesh_load(verts, src, f64);
    o[1] = (float)mesh_load(verts, src + 1, f64);
    o[2] = (float)mesh_load(verts, src + 2, f64);
    o[3] = nx;
    o[4] = ny;
    o[5] = nz;
  }
  if (out_normals) {
    float* o = out_normals + row * 3;
    o[0] = nx;
    o[1] = ny;
    o[2] = nz;
  }
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_area_kernel(const void* __restrict__ verts, int f64, int64_t n_vertices, int64_t n_faces,
                                                                 const int32_t* __restrict__ faces, double* __restrict__ out_areas,
                                                                 int32_t* __restrict__ flag) {
#pragma clang fp contract(off)
  const int64_t f = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (f >= n_faces) return;
  double area = 0.0;
  int i0, i1, i2;
  if (face_indices(faces + 3 * f, n_vertices, flag, i0, i1, i2)) {
    const vec3 v0 = mesh_vertex(verts, 0, i0, f64), v1 = mesh_vertex(verts, 0, i1, f64), v2 = mesh_vertex(verts, 0, i2, f64);
    area = norm3(cross3(sub3(v1, v0), sub3(v2, v0))) / 2.0;
  }
  out_areas[f] = area;
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_sample_kernel(const void* __restrict__ verts, int f64, int64_t n_vertices, int64_t n_faces,
                                                                   const int32_t* __restrict__ faces, const double* __restrict__ cdf,
                                                                   int64_t n_samples, const double* __restrict__ u_face,
                                                                   const double* __restrict__ u_bary, double* __restrict__ out_points,
                                                                   int32_t* __restrict__ out_face_index, double* __restrict__ out_normals,
                                                                   int32_t* __restrict__ flag) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (i >= n_samples) return;
  const double pick = u_face[i] * cdf[n_faces - 1];
  // np.searchsorted(cdf, pick), side left: the first index with cdf[index] >= pick; lo stays inside [0, n_faces - 1] whatever
  // the values are (a NaN compares false and the search ends on the last face)
  int64_t lo = 0, hi = n_faces - 1;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (cdf[mid] >= pick)
      hi = mid;
    else
      lo = mid + 1;
  }
  const int64_t f = lo;
  out_face_index[i] = (int32_t)f;
  double r0 = u_bary[2 * i], r1 = u_bary[2 * i + 1];
  if (r0 + r1 > 1.0) {
    r0 = r0 - 1.0;
    r1 = r1 - 1.0;
  }
  r0 = fabs(r0);
  r1 = fabs(r1);
  vec3 p = {0.0, 0.0, 0.0}, n = {0.0, 0.0, 0.0};
  int i0, i1, i2;
  if (face_indices(faces + 3 * f, n_vertices, flag, i0, i1, i2)) {
    const vec3 v0 = mesh_vertex(verts, 0, i0, f64), v1 = mesh_vertex(verts, 0, i1, f64), v2 = mesh_vertex(verts, 0, i2, f64);
    const vec3 e1 = sub3(v1, v0), e2 = sub3(v2, v0);
    p.x = (v0.x + e1.x * r0) + e2.x * r1;
    p.y = (v0.y + e1.y * r0) + e2.y * r1;
    p.z = (v0.z + e1.z * r0) + e2.z * r1;
    if (out_normals) {
      const vec3 c = cross3(e1, e2);
      n = unit_normal(c, norm3(c));
    }
  }
  out_points[3 * i] = p.x;
  out_points[3 * i + 1] = p.y;
  out_points[3 * i + 2] = p.z;
  if (out_normals) {
    out_normals[3 * i] = n.x;
    out_normals[3 * i + 1] = n.y;
    out_normals[3 * i + 2] = n.z;
  }
}

}  // namespace

// staged { unit normal, three corner angles }: double[n_frames][n_faces][6]
extern "C" size_t am_vertex_normals_workspace_bytes(int n_frames, int64_t n_faces) {
  if (n_frames < 1 || n_faces < 1 || n_faces > MESH_MAX) return 0;
  return (size_t)n_frames * (size_t)n_faces * 6 * sizeof(double);
}

extern "C" int am_vertex_normals(const am_vertex_normals_args* a, void* stream) {
  AM_CHECK(a != nullptr, "am_vertex_normals: null arguments");
  AM_CHECK(a->n_frames >= 1 && a->n_frames <= 65535, "am_vertex_normals: %d frames outside 1 .. 65535", a->n_frames);
  AM_TRY(check_mesh("am_vertex_normals", a->n_vertices, a->n_faces, 0));
  AM_CHECK(a->vertices_f64 == 0 || a->vertices_f64 == 1, "am_vertex_normals: vertices_f64 must be 0 or 1, got %d", a->vertices_f64);
  AM_CHECK(a->frame_stride >= 3 * a->n_vertices || a->n_frames == 1, "am_vertex_normals: frame stride %lld below 3 * %lld vertices",
           (long long)a->frame_stride, (long long)a->n_vertices);
  AM_CHECK(a->vertices && a->offsets && a->out_flag && (a->n_faces == 0 || (a->faces && a->corners)), "am_vertex_normals: null pointer");
  AM_CHECK(a->out_features || a->out_normals || a->out_face_normals, "am_vertex_normals: no output requested");
  const size_t need = am_vertex_normals_workspace_bytes(a->n_frames, a->n_faces);
  AM_CHECK(need == 0 || (a->workspace != nullptr && a->workspace_bytes >= need),
           "am_vertex_normals: workspace of %zu bytes needed, %zu given", need, (size_t)a->workspace_bytes);
  AM_CHECK((reinterpret_cast<uintptr_t>(a->workspace) & 15) == 0, "am_vertex_normals: the workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  double* staged = reinterpret_cast<double*>(a->workspace);
  const int64_t stride = a->n_frames == 1 ? 0 : a->frame_stride;
  AM_HIP(hipMemsetAsync(a->out_flag, 0, sizeof(int32_t), st));
  if (a->n_faces > 0)
    hipLaunchKernelGGL(mesh_face_kernel, dim3(mesh_blocks(a->n_faces), a->n_frames), dim3(MESH_THREADS), 0, st, a->vertices,
                       (int)a->vertices_f64, stride, a->n_vertices, a->n_faces, a->faces, staged, a->out_face_normals, a->out_flag);
  if (a->out_features || a->out_normals) {
    const mesh_view m = {a->n_vertices, a->n_faces, 0, a->faces, a->offsets, a->corners, nullptr, nullptr, a->out_flag};
    hipLaunchKernelGGL(mesh_vertex_kernel, dim3(mesh_blocks(a->n_vertices), a->n_frames), dim3(MESH_THREADS), 0, st, m, a->vertices,
                       (int)a->vertices_f64, stride, staged, a->out_features, a->out_normals);
  }
  AM_HIP(hipGetLastError());
  return AM_OK;
}

extern "C" int am_face_areas(const am_face_areas_args* a, void* stream) {
  AM_CHECK(a != nullptr, "am_face_areas: null arguments");
  AM_TRY(check_mesh("am_face_areas", a->n_vertices, a->n_faces));
  AM_CHECK(a->vertices_f64 == 0 || a->vertices_f64 == 1, "am_face_areas: vertices_f64 must be 0 or 1, got %d", a->vertices_f64);
  AM_CHECK(a->vertices && a->faces && a->out_areas && a->out_flag, "am_face_areas: null pointer");
  hipStream_t st = (hipStream_t)stream;
  AM_HIP(hipMemsetAsync(a->out_flag, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(mesh_area_kernel, dim3(mesh_blocks(a->n_faces)), dim3(MESH_THREADS), 0, st, a->vertices, (int)a->vertices_f64,
                     a->n_vertices, a->n_faces, a->faces, a->out_areas, a->out_flag);
  AM_HIP(hipGetLastError());
  return AM_OK;
}

extern "C" int am_surface_sample(const am_surface_sample_args* a, void* stream) {
  AM_CHECK(a != nullptr, "am_surface_sample: null arguments");
  AM_TRY(check_mesh("am_surface_sample", a->n_vertices, a->n_faces));
  AM_CHECK(a->n_samples >= 1 && a->n_samples <= MESH_MAX, "am_surface_sample: %lld samples outside 1 .. (2^31 - 1) / 3",
           (long long)a->n_samples);
  AM_CHECK(a->vertices_f64 == 0 || a->vertices_f64 == 1, "am_surface_sample: vertices_f64 must be 0 or 1, got %d", a->vertices_f64);
  AM_CHECK(a->vertices && a->faces && a->cdf && a->u_face && a->u_bary && a->out_points && a->out_face_index && a->out_flag,
           "am_surface_sample: null pointer");
  hipStream_t st = (hipStream_t)stream;
  AM_HIP(hipMemsetAsync(a->out_flag, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(mesh_sample_kernel, dim3(mesh_blocks(a->n_samples)), dim3(MESH_THREADS), 0, st, a->vertices, (int)a->vertices_f64,
                     a->n_vertices, a->n_faces, a->faces, a->cdf, a->n_samples, a->u_face, a->u_bary, a->out_points, a->out_face_index,
                     a->out_normals, a->out_flag);
  AM_HIP(hipGetLastError());
  return AM_OK;
}
