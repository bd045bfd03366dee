// Normal-map preview renderer: the arithmetic of the reference's preview video (actionmesh/render/renderer.py - PyTorch3D's
// MeshRasterizer with bin_size=0, blur 0, one face per pixel, perspective-correct clipped barycentrics - followed by
// soft_normal_shading and make_normal_image), for every (frame, camera) image of one animated mesh in a fixed number of launches.
//
//   vertex normals       one thread per (frame, vertex): sum of cross(v2 - v1, v0 - v1) over its faces, normalised (eps 1e-6).  Its
//                        faces are corner / 3 along the caller's vertex -> corner CSR (am_vertex_normals' table: ascending corner
//                        id), so every sum is in face-index order;
//   projection           one thread per (frame, camera, vertex): {x_ndc, y_ndc, view z};
//   raster               one thread per (image, face): a face whose pixel bounding box holds at most SMALL_BOX sub-pixels
//                        tests them itself; a larger one is queued, and raster_big spreads each queued face over BIG_SPLIT
//                        blocks of 256 threads (a frame-filling quad does not serialise one lane).  The z-buffer is one
//                        64-bit word per sub-pixel, (depth bits << 32) | face, lowered by atomicMin: depth >= 0 orders like
//                        its bits, so the nearest face wins and ties go to the lowest face index, whatever the arrival order;
//   resolve              one thread per output pixel: mask from the 2 x 2 sub-pixels, normal from sub-pixel (2i, 2j).
// The coverage test is a function of (face, sub-pixel) alone, evaluated by the same code in raster and resolve, without
// contraction: the result is bit-identical run to run and independent of how the images are batched.  Faces and CSR are read
// through am_geometry.h: every index is compared with its bound before it is an address, and a bad one raises the call's flag.
#include "am_geometry.h"

namespace {

constexpr int RT_THREADS = 256;
constexpr int SMALL_BOX = 64;        // sub-pixels a raster thread tests itself
constexpr int BIG_BLOCKS = 1024;     // raster_big: blocks striding over the queue ...
constexpr int BIG_SPLIT = 8;         // ... times blocks sharing one queued face
constexpr float K_EPS = 1e-8f;       // PyTorch3D's kEpsilon (rasterize_meshes)
constexpr unsigned long long ZB_EMPTY = ~0ull;

struct RenderCams { am_render_camera c[AM_RENDER_MAX_CAMERAS]; };

__device__ inline float edge_fn(float px, float py, float ax, float ay, float bx, float by) {
#pragma clang fp contract(off)
  return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}

// PyTorch3D's CheckPixelInsideFace for blur 0 and clipped, perspective-correct barycentrics: true when (px, py) is covered;
// then b = the clipped barycentrics and z = the interpolated depth (>= 0).  A centre outside the closed bounding box of the three
// projected vertices is never covered (PyTorch3D's rule as remembered, unpinned): that is decided here, exactly, so that it does not
// depend on the loop bounds of pix_range.  Only a face with a vertex behind the camera has barycentrics > 0 outside its box.
__device__ inline bool cover(const float4& v0, const float4& v1, const float4& v2, float px, float py, float b[3], float& z) {
#pragma clang fp contract(off)
  if (px < fminf(fminf(v0.x, v1.x), v2.x) || px > fmaxf(fmaxf(v0.x, v1.x), v2.x) || py < fminf(fminf(v0.y, v1.y), v2.y) ||
      py > fmaxf(fmaxf(v0.y, v1.y), v2.y))
    return false;
  const float area = edge_fn(v2.x, v2.y, v0.x, v0.y, v1.x, v1.y) + K_EPS;
  const float w0 = edge_fn(px, py, v1.x, v1.y, v2.x, v2.y) / area;
  const float w1 = edge_fn(px, py, v2.x, v2.y, v0.x, v0.y) / area;
  const float w2 = edge_fn(px, py, v0.x, v0.y, v1.x, v1.y) / area;
  const float t0 = w0 * v1.z * v2.z, t1 = v0.z * w1 * v2.z, t2 = v0.z * v1.z * w2;
  const float den = fmaxf(t0 + t1 + t2, K_EPS);
  const float p0 = t0 / den, p1 = t1 / den, p2 = t2 / den;
  if (!(p0 > 0.f && p1 > 0.f && p2 > 0.f)) return false;
  const float c0 = fmaxf(p0, 0.f), c1 = fmaxf(p1, 0.f), c2 = fmaxf(p2, 0.f);
  const float s = fmaxf(c0 + c1 + c2, 1e-5f);
  b[0] = c0 / s;
  b[1] = c1 / s;
  b[2] = c2 / s;
  z = b[0] * v0.z + b[1] * v1.z + b[2] * v2.z;
  return z >= 0.f;                   // also false for NaN
}

__device__ inline float ndc_of(int i, int n) { return 1.f - (float)(2 * i + 1) / (float)n; }

// the sub-pixel range [lo, hi] whose centres can lie in [a_min, a_max] of NDC (conservative by one sub-pixel; NaN / inf -> all):
// a loop bound only - cover() decides with the exact box
__device__ inline void pix_range(float a_min, float a_max, int n, int& lo, int& hi) {
  const float f_lo = ((1.f - a_max) * (float)n - 1.f) * 0.5f, f_hi = ((1.f - a_min) * (float)n - 1.f) * 0.5f;
  lo = !(f_lo > 1.f) ? 0 : (f_lo >= (float)n ? n : (int)f_lo - 1);
  hi = !(f_hi < (float)(n - 2)) ? n - 1 : (f_hi < -1.f ? -1 : (int)f_hi + 1);
}

struct FaceSetup {
  float4 v0, v1, v2;
  int r_lo, r_hi, c_lo, c_hi;
};

// PyTorch3D's per-face rejections (every vertex behind the camera, |area| <= 1e-8, index outside the mesh) and the bounding box.
__device__ inline bool face_setup(const int32_t* __restrict__ faces, const float4* __restrict__ proj, int f, int V, int W,
                                  int32_t* __restrict__ flag, FaceSetup& s) {
#pragma clang fp contract(off)
  __builtin_assume(V > 0);           // render_check; each range test is then one unsigned compare and the three index loads stay together
  int i0, i1, i2;
  if (!face_indices(faces + 3 * f, V, flag, i0, i1, i2)) return false;
  s.v0 = proj[i0];
  s.v1 = proj[i1];
  s.v2 = proj[i2];
  if (fmaxf(fmaxf(s.v0.z, s.v1.z), s.v2.z) < 0.f) return false;
  const float a = edge_fn(s.v0.x, s.v0.y, s.v1.x, s.v1.y, s.v2.x, s.v2.y);
  if (a <= K_EPS && a >= -K_EPS) return false;
  pix_range(fminf(fminf(s.v0.x, s.v1.x), s.v2.x), fmaxf(fmaxf(s.v0.x, s.v1.x), s.v2.x), W, s.c_lo, s.c_hi);
  pix_range(fminf(fminf(s.v0.y, s.v1.y), s.v2.y), fmaxf(fmaxf(s.v0.y, s.v1.y), s.v2.y), W, s.r_lo, s.r_hi);
  return s.c_lo <= s.c_hi && s.r_lo <= s.r_hi;
}

__device__ inline void zb_test(unsigned long long* __restrict__ zb, const FaceSetup& s, int f, int r, int c, int W) {
  float b[3], z;
  if (!cover(s.v0, s.v1, s.v2, ndc_of(c, W), ndc_of(r, W), b, z)) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(z > 0.f ? z : 0.f) << 32) | (unsigned)f;
  unsigned long long* p = zb + (int64_t)r * W + c;
  if (key < *p) atomicMin(p, key);   // the plain read only filters: atomicMin decides
}

// ---- per-frame vertex normals and per-(frame, camera) projection ----------------------------------------------------------
__global__ void vnormal_kernel(mesh_view m, const float* __restrict__ X, int64_t TV, float* __restrict__ vn) {
#pragma clang fp contract(off)
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= TV) return;
  const int v = (int)(g % m.n_vertices);
  const float* Xt = X + (g - v) * 3;
  float nx = 0.f, ny = 0.f, nz = 0.f;
  int begin, end;
  csr_range(m, v, begin, end);
  for (int j = begin; j < end; ++j) {
    const int c = corner_at(m, j, v);
    int i0, i1, i2;
    if (c < 0 || !face_indices(m.faces + 3 * (c / 3), m.n_vertices, m.flag, i0, i1, i2)) continue;
    const float *p0 = Xt + 3 * i0, *p1 = Xt + 3 * i1, *p2 = Xt + 3 * i2;
    const float ax = p2[0] - p1[0], ay = p2[1] - p1[1], az = p2[2] - p1[2];
    const float bx = p0[0] - p1[0], by = p0[1] - p1[1], bz = p0[2] - p1[2];
    nx += ay * bz - az * by;
    ny += az * bx - ax * bz;
    nz += ax * by - ay * bx;
  }
  const float d = fmaxf(sqrtf(nx * nx + ny * ny + nz * nz), 1e-6f);
  vn[g * 3 + 0] = nx / d;
  vn[g * 3 + 1] = ny / d;
  vn[g * 3 + 2] = nz / d;
}

__global__ void project_kernel(const float* __restrict__ X, int V, int C, RenderCams cams, float4* __restrict__ proj) {
#pragma clang fp contract(off)
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  const int img = blockIdx.y;
  if (v >= V) return;
  const am_render_camera& cm = cams.c[img % C];
  const float* p = X + ((int64_t)(img / C) * V + v) * 3;
  float q[3];
  for (int j = 0; j < 3; ++j) q[j] = p[0] * cm.R[j] + p[1] * cm.R[3 + j] + p[2] * cm.R[6 + j] + cm.T[j];
  proj[(int64_t)img * V + v] = make_float4(cm.fx * q[0] / q[2] + cm.px, cm.fy * q[1] / q[2] + cm.py, q[2], 0.f);
}

// ---- rasterisation --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RT_THREADS) void raster_small_kernel(const int32_t* __restrict__ faces, const float4* __restrict__ proj,
                                                                  int V, int F, int W, unsigned long long* __restrict__ zb,
                                                                  unsigned* __restrict__ queue, int32_t* __restrict__ flag) {
  const int f = blockIdx.x * RT_THREADS + threadIdx.x;
  const int img = blockIdx.y;
  if (f >= F) return;
  FaceSetup s;
  if (!face_setup(faces, proj + (int64_t)img * V, f, V, W, flag, s)) return;
  const int bw = s.c_hi - s.c_lo + 1;
  if ((int64_t)bw * (s.r_hi - s.r_lo + 1) > SMALL_BOX) {
    queue[1 + atomicAdd(queue, 1u)] = (unsigned)img * (unsigned)F + (unsigned)f;
    return;
  }
  unsigned long long* z = zb + (int64_t)img * W * W;
  for (int r = s.r_lo; r <= s.r_hi; ++r)
    for (int c = s.c_lo; c <= s.c_hi; ++c) zb_test(z, s, f, r, c, W);
}

__global__ __launch_bounds__(RT_THREADS) void raster_big_kernel(const int32_t* __restrict__ faces, const float4* __restrict__ proj,
                                                                int V, int F, int W, unsigned long long* __restrict__ zb,
                                                                const unsigned* __restrict__ queue, int32_t* __restrict__ flag) {
  const unsigned n = queue[0];
  for (unsigned e = blockIdx.x; e < n; e += gridDim.x) {
    const unsigned code = queue[1 + e];
    const int img = (int)(code / (unsigned)F), f = (int)(code % (unsigned)F);
    FaceSetup s;
    if (!face_setup(faces, proj + (int64_t)img * V, f, V, W, flag, s)) continue;
    const int bw = s.c_hi - s.c_lo + 1;
    const int64_t area = (int64_t)bw * (s.r_hi - s.r_lo + 1);
    unsigned long long* z = zb + (int64_t)img * W * W;
    for (int64_t p = (int64_t)blockIdx.y * RT_THREADS + threadIdx.x; p < area; p += (int64_t)gridDim.y * RT_THREADS)
      zb_test(z, s, f, s.r_lo + (int)(p / bw), s.c_lo + (int)(p % bw), W);
  }
}

// ---- resolve ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RT_THREADS) void resolve_kernel(const int32_t* __restrict__ faces, const float4* __restrict__ proj,
                                                             const float* __restrict__ vn, const unsigned long long* __restrict__ zb,
                                                             int V, int C, int S, RenderCams cams, uint8_t* __restrict__ out_rgba,
                                                             float* __restrict__ out_mask, float* __restrict__ out_normal,
                                                             int32_t* __restrict__ out_face, float* __restrict__ out_bary,
                                                             int32_t* __restrict__ flag) {
#pragma clang fp contract(off)
  const int pix = blockIdx.x * RT_THREADS + threadIdx.x;
  const int img = blockIdx.y;
  if (pix >= S * S) return;
  const int i = pix / S, j = pix % S, W = 2 * S;
  const int64_t sub0 = (int64_t)img * W * W;
  const float4* pr = proj + (int64_t)img * V;
  int covered = 0;
  float n[3] = {0.f, 0.f, 0.f};
  for (int k = 0; k < 4; ++k) {
    const int r = 2 * i + (k >> 1), c = 2 * j + (k & 1);
    const unsigned long long key = zb[sub0 + (int64_t)r * W + c];
    const int f = key == ZB_EMPTY ? -1 : (int)(unsigned)(key & 0xffffffffu);
    covered += f >= 0;
    float b[3] = {-1.f, -1.f, -1.f};
    int i0, i1, i2;
    if (f >= 0 && (k == 0 || out_bary) && face_indices(faces + 3 * f, V, flag, i0, i1, i2)) {     // a face the raster accepted
      float z;
      cover(pr[i0], pr[i1], pr[i2], ndc_of(c, W), ndc_of(r, W), b, z);      // the raster's own test: covered again
      if (k == 0) {
        const float* vt = vn + (int64_t)(img / C) * V * 3;
        for (int a = 0; a < 3; ++a) n[a] = b[0] * vt[3 * i0 + a] + b[1] * vt[3 * i1 + a] + b[2] * vt[3 * i2 + a];
      }
    }
    if (out_face) out_face[sub0 + (int64_t)r * W + c] = f;
    if (out_bary)
      for (int a = 0; a < 3; ++a) out_bary[(sub0 + (int64_t)r * W + c) * 3 + a] = b[a];
  }
  // soft_normal_shading: the world-to-view transform of the camera with T halved, applied to the normal as to a point
  const am_render_camera& cm = cams.c[img % C];
  float m[3];
  for (int a = 0; a < 3; ++a) m[a] = n[0] * cm.R[a] + n[1] * cm.R[3 + a] + n[2] * cm.R[6 + a] + cm.T[a] * 0.5f;
  const float d = fmaxf(sqrtf(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]), 1e-12f);
  const float mask = (float)covered * 0.25f;
  const int64_t o = (int64_t)img * S * S + pix;
  uint8_t px[4];
  for (int a = 0; a < 3; ++a) {
    const float u = fminf(fmaxf((m[a] / d + 1.f) * 0.5f, 0.f), 1.f);
    if (out_normal) out_normal[o * 3 + a] = u;
    px[a] = (uint8_t)((u * mask + (1.f - mask)) * 255.f);
  }
  px[3] = (uint8_t)(mask * 255.f);
  *reinterpret_cast<uchar4*>(out_rgba + o * 4) = make_uchar4(px[0], px[1], px[2], px[3]);
  if (out_mask) out_mask[o] = mask;
}

struct RenderLayout { size_t vn, proj, zb, queue, total; };

RenderLayout render_layout(int T, int V, int F, int C, int S) {
  auto a = [](size_t x) { return (x + 255) / 256 * 256; };
  RenderLayout l;
  const size_t imgs = (size_t)T * C, W = 2 * (size_t)S;
  l.vn = 0;
  l.proj = l.vn + a(sizeof(float) * 3 * (size_t)T * V);
  l.zb = l.proj + a(sizeof(float4) * imgs * V);
  l.queue = l.zb + a(sizeof(unsigned long long) * imgs * W * W);
  l.total = l.queue + a(sizeof(unsigned) * (1 + imgs * F));
  return l;
}

int render_check(const am_render_args* a) {
  AM_CHECK(a != nullptr, "am_render_normals: null arguments");
  AM_CHECK(a->n_frames >= 1 && a->n_verts >= 1 && a->n_faces >= 1, "am_render_normals: empty problem (%d frames, %d vertices, %d faces)",
           a->n_frames, a->n_verts, a->n_faces);
  AM_CHECK(a->n_cameras >= 1 && a->n_cameras <= AM_RENDER_MAX_CAMERAS, "am_render_normals: %d cameras, 1 .. %d supported",
           a->n_cameras, AM_RENDER_MAX_CAMERAS);
  AM_CHECK(a->image_size >= 1 && a->image_size <= 4096, "am_render_normals: image size %d outside 1 .. 4096", a->image_size);
  AM_CHECK(a->verts && a->faces && a->offsets && a->corners && a->out_flag && a->out_rgba, "am_render_normals: null pointer");
  const int64_t imgs = (int64_t)a->n_frames * a->n_cameras;
  AM_CHECK(imgs <= 65535, "am_render_normals: %lld images exceed the grid's y extent", (long long)imgs);
  AM_CHECK((int64_t)a->n_frames * a->n_verts < ((int64_t)1 << 31) / 3, "am_render_normals: %d x %d vertices overflow a 32-bit index",
           a->n_frames, a->n_verts);
  AM_CHECK(imgs * a->n_faces < ((int64_t)1 << 32) - 1, "am_render_normals: %lld images x %d faces overflow the raster queue",
           (long long)imgs, a->n_faces);
  AM_CHECK((int64_t)a->n_faces * 3 < ((int64_t)1 << 31), "am_render_normals: %d faces overflow a 32-bit index", a->n_faces);
  return AM_OK;
}

}  // namespace

extern "C" size_t am_render_workspace_bytes(int n_frames, int n_verts, int n_faces, int n_cameras, int image_size) {
  if (n_frames < 1 || n_verts < 1 || n_faces < 1 || n_cameras < 1 || image_size < 1) return 0;
  return render_layout(n_frames, n_verts, n_faces, n_cameras, image_size).total;
}

extern "C" int am_render_normals(const am_render_args* a, void* workspace_dev, size_t workspace_bytes, void* stream) {
  AM_TRY(render_check(a));
  const int T = a->n_frames, V = a->n_verts, F = a->n_faces, C = a->n_cameras, S = a->image_size, W = 2 * S;
  const RenderLayout l = render_layout(T, V, F, C, S);
  AM_CHECK(workspace_dev != nullptr && workspace_bytes >= l.total, "am_render_normals: workspace of %zu bytes needed, %zu given",
           l.total, workspace_bytes);
  hipStream_t st = (hipStream_t)stream;
  char* ws = reinterpret_cast<char*>(workspace_dev);
  float* vn = reinterpret_cast<float*>(ws + l.vn);
  float4* proj = reinterpret_cast<float4*>(ws + l.proj);
  unsigned long long* zb = reinterpret_cast<unsigned long long*>(ws + l.zb);
  unsigned* queue = reinterpret_cast<unsigned*>(ws + l.queue);
  const int imgs = T * C;
  RenderCams cams;
  for (int c = 0; c < AM_RENDER_MAX_CAMERAS; ++c) cams.c[c] = a->cameras[c];

  const mesh_view m = {V, F, 0, a->faces, a->offsets, a->corners, nullptr, nullptr, a->out_flag};
  AM_HIP(hipMemsetAsync(a->out_flag, 0, sizeof(int32_t), st));
  AM_HIP(hipMemsetAsync(zb, 0xff, sizeof(unsigned long long) * (size_t)imgs * W * W, st));
  AM_HIP(hipMemsetAsync(queue, 0, sizeof(unsigned), st));
  const int64_t TV = (int64_t)T * V;
  hipLaunchKernelGGL(vnormal_kernel, dim3(ceil_div(TV, 256)), dim3(256), 0, st, m, a->verts, TV, vn);
  AM_HIP(hipGetLastError());
  hipLaunchKernelGGL(project_kernel, dim3(ceil_div(V, 256), imgs), dim3(256), 0, st, a->verts, V, C, cams, proj);
  AM_HIP(hipGetLastError());
  hipLaunchKernelGGL(raster_small_kernel, dim3(ceil_div(F, RT_THREADS), imgs), dim3(RT_THREADS), 0, st, a->faces, proj, V, F, W, zb,
                     queue, a->out_flag);
  AM_HIP(hipGetLastError());
  hipLaunchKernelGGL(raster_big_kernel, dim3(BIG_BLOCKS, BIG_SPLIT), dim3(RT_THREADS), 0, st, a->faces, proj, V, F, W, zb, queue,
                     a->out_flag);
  AM_HIP(hipGetLastError());
  hipLaunchKernelGGL(resolve_kernel, dim3(ceil_div((int64_t)S * S, RT_THREADS), imgs), dim3(RT_THREADS), 0, st, a->faces, proj, vn, zb,
                     V, C, S, cams, a->out_rgba, a->out_mask, a->out_normal, a->out_face, a->out_bary, a->out_flag);
  AM_HIP(hipGetLastError());
  return AM_OK;
}
