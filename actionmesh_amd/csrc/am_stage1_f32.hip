// The row / elementwise kernels of the exact-fp32 Stage-I denoiser (HipDenoiser(dtype="float32"), actionmesh_amd/denoiser_f32.py)
// and of the exact-fp32 Stage-II decoder (HipAutoencoder(exact_fp32=True), actionmesh_amd/autoencoder_f32.py) that the exact-fp32
// matrix path of am_f32.hip does not have:
//   am_head_post_f32   qk-RMSNorm (+ RoPE) in place on a packed fp32 projection output      (attention_processor.py:121-130)
//   am_rope_f32        RoPE alone, q and k chunks in one launch (Stage II has no qk-norm)     (attention_processor.py:127-130)
//   am_flow_step_f32   classifier-free guidance + Euler step on an fp32 velocity             (guidance.py:95-118, scheduler.py:238-248)
// fp32 and nothing narrower; every operation is rounded once, in the order include/actionmesh_amd.h writes it: the file is built
// without the SLP vectoriser and WITHOUT contraction into fused multiply-adds (csrc/Makefile), so am_flow_step_f32 gives the bits of
// the torch fp32 expression, and am_rope_f32 those of the unfused torch fp32 rotation.  Nothing here depends on the 16-bit type: both
// library builds carry the same object code.  The kernels are HBM-bound: 16-byte accesses, no LDS, no scratch.
#include "am_common.h"

namespace {

constexpr int HP_D = 128;          // head_dim: one 128-float chunk = 32 lanes x float4 = half a wave
constexpr int HP_CHUNKS = 8;       // chunks per 256-thread workgroup

// The lane's four floats of the chunk at column `col` of row `row`: the interleaved pairs 2 lane and 2 lane + 1 of the chunk.  *t: where
// the angles of those two pairs stand in the (frames, 64) tables - every row of a frame shares the frame's angles.
__device__ __forceinline__ float* chunk_ptr(float* X, int64_t ldx, int64_t row, int64_t col, int rows_per_frame, int lane, int64_t* t) {
  *t = (row / rows_per_frame) * (HP_D / 2) + 2 * lane;
  return X + row * ldx + col + 4 * lane;
}

// rotary_embedding.py:72-124 on the lane's two pairs: out = x cos + rot(x) sin, rot(x)[2i] = -x[2i + 1], rot(x)[2i + 1] = x[2i] - two
// products and one sum per element, each rounded once (the file is built without contraction)
__device__ __forceinline__ f32x4_t rotate_pairs(f32x4_t x, const float* rope_cos, const float* rope_sin, int64_t t) {
  const float c0 = rope_cos[t], c1 = rope_cos[t + 1], s0 = rope_sin[t], s1 = rope_sin[t + 1];
  return f32x4_t{x[0] * c0 + (-x[1]) * s0, x[1] * c0 + x[0] * s0, x[2] * c1 + (-x[3]) * s1, x[3] * c1 + x[2] * s1};
}

struct HeadPostF32 {
  float* X; int64_t ldx; int off, head_stride;
  int64_t chunks; int heads;
  const float* w; float eps;
  const float* rope_cos; const float* rope_sin; int rows_per_frame;
};

// One (row, head) chunk per half wave.  Sum of squares: the lane's four squares pairwise, then five xor-shuffle levels inside the
// half wave - a tree of 1 (square) + 2 + 5 = 8 levels, the same tree for every chunk of every launch.
__global__ __launch_bounds__(256) void head_post_f32_kernel(HeadPostF32 p) {
  const int lane = threadIdx.x & 31;
  const int64_t chunk = (int64_t)blockIdx.x * HP_CHUNKS + (threadIdx.x >> 5);
  const bool valid = chunk < p.chunks;
  const int64_t row = valid ? chunk / p.heads : 0;
  const int head = valid ? (int)(chunk - row * p.heads) : 0;
  int64_t t;
  float* xp = chunk_ptr(p.X, p.ldx, row, p.off + (int64_t)head * p.head_stride, p.rows_per_frame, lane, &t);
  f32x4_t x = valid ? *reinterpret_cast<const f32x4_t*>(xp) : f32x4_t{0.f, 0.f, 0.f, 0.f};
  float ss = (x[0] * x[0] + x[1] * x[1]) + (x[2] * x[2] + x[3] * x[3]);
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
  const float r = 1.0f / sqrtf(ss * (1.0f / HP_D) + p.eps);          // torch.rsqrt(mean + eps); the division by 128 is exact
  const f32x4_t wv = *reinterpret_cast<const f32x4_t*>(p.w + 4 * lane);
  f32x4_t y;
#pragma unroll
  for (int e = 0; e < 4; ++e) y[e] = x[e] * r * wv[e];
  if (p.rope_cos) y = rotate_pairs(y, p.rope_cos, p.rope_sin, t);
  if (valid) *reinterpret_cast<f32x4_t*>(xp) = y;
}

struct RopeF32 {
  float* X; int64_t ldx; int off[2]; int head_stride;
  int64_t chunks; int heads, kinds;
  const float* rope_cos; const float* rope_sin; int rows_per_frame;
};

// One (row, kind, head) chunk per half wave, kind 0 = the chunks at off[0] (q), kind 1 = those at off[1] (k): the chunks of one row are
// neighbours in the grid.  No reduction, so a half wave past the last chunk simply leaves.
__global__ __launch_bounds__(256) void rope_f32_kernel(RopeF32 p) {
  const int lane = threadIdx.x & 31;
  const int64_t chunk = (int64_t)blockIdx.x * HP_CHUNKS + (threadIdx.x >> 5);
  if (chunk >= p.chunks) return;
  const int per_row = p.kinds * p.heads;
  const int64_t row = chunk / per_row;
  const int in_row = (int)(chunk - row * per_row);
  const int kind = in_row / p.heads, head = in_row - kind * p.heads;
  int64_t t;
  float* xp = chunk_ptr(p.X, p.ldx, row, p.off[kind] + (int64_t)head * p.head_stride, p.rows_per_frame, lane, &t);
  *reinterpret_cast<f32x4_t*>(xp) = rotate_pairs(*reinterpret_cast<const f32x4_t*>(xp), p.rope_cos, p.rope_sin, t);
}

struct FlowF32 {
  const float* v; float* lat; int nb; float scales[3]; float dt; int additive;
  uint8_t unobs[256]; int64_t per_frame4, total4;       // in float4 units
};

// One element of the step: `lat` its latent, `v0` branch 0's velocity, branch(b) that of branch b = 1 .. nb - 1
template <class Branch>
__device__ __forceinline__ float flow_element(const FlowF32& a, float lat, float v0, Branch branch) {
  float o = v0, prev = o;
#pragma unroll
  for (int b = 1; b < 4; ++b) {
    if (b < a.nb) {
      const float c = branch(b);
      o = o + a.scales[b - 1] * (c - prev);            // guidance.py:113-116: output += scale_i * (v_{i+1} - v_i)
      prev = c;
    }
  }
  const float step = a.dt * o;                         // scheduler.py:238-241: distances[i] * output_pred
  return a.additive ? lat + step : lat - step;
}

// VEC: one float4 of the latents per thread; otherwise (a frame size that is no multiple of 4) one element per thread
template <bool VEC>
__global__ __launch_bounds__(256) void flow_step_f32_kernel(FlowF32 a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.total4) return;
  if (!a.unobs[(int)(i / a.per_frame4)]) return;
  if (VEC) {
    const f32x4_t* v = reinterpret_cast<const f32x4_t*>(a.v);
    f32x4_t* lat = reinterpret_cast<f32x4_t*>(a.lat);
    f32x4_t cur[3];
#pragma unroll
    for (int b = 1; b < 4; ++b) cur[b - 1] = b < a.nb ? v[(int64_t)b * a.total4 + i] : f32x4_t{0.f, 0.f, 0.f, 0.f};
    f32x4_t x = lat[i];
    const f32x4_t v0 = v[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = flow_element(a, x[e], v0[e], [&](int b) { return cur[b - 1][e]; });
    lat[i] = x;
  } else {
    a.lat[i] = flow_element(a, a.lat[i], a.v[i], [&](int b) { return a.v[(int64_t)b * a.total4 + i]; });
  }
}

// the (frames, 64) tables reach the frame of the last row
inline bool frames_cover(int64_t rows, int rows_per_frame, int frames) {
  return rows_per_frame > 0 && frames > 0 && (rows - 1) / rows_per_frame < frames;
}

}  // namespace

extern "C" int am_head_post_f32(float* X, int64_t ldx, int off, int head_stride, int64_t rows, int heads, const float* w, float eps,
                                const float* rope_cos, const float* rope_sin, int frames, int rows_per_frame, void* stream) {
  AM_CHECK(X && w, "am_head_post_f32: null operand");
  AM_CHECK(rows > 0 && heads > 0 && heads <= 65535, "am_head_post_f32: bad shape rows=%lld heads=%d", (long long)rows, heads);
  AM_CHECK(al16(X) && al16(w) && heads_aligned(ldx, off, head_stride),
           "am_head_post_f32: X, w, ldx, off and head_stride must be 16-byte aligned");
  AM_CHECK((heads == 1 || head_stride >= HP_D) && heads_fit(ldx, off, head_stride, heads, HP_D),
           "am_head_post_f32: the heads' chunks overlap or run past the row (ldx=%lld off=%d head_stride=%d heads=%d)", (long long)ldx,
           off, head_stride, heads);
  AM_CHECK((rope_cos == nullptr) == (rope_sin == nullptr), "am_head_post_f32: rope tables must come in pairs");
  if (rope_cos)
    AM_CHECK(frames_cover(rows, rows_per_frame, frames),
             "am_head_post_f32: rows=%lld / rows_per_frame=%d runs past the %d frames of the tables", (long long)rows, rows_per_frame, frames);
  const int64_t chunks = rows * heads, blocks = (chunks + HP_CHUNKS - 1) / HP_CHUNKS;
  AM_CHECK(blocks <= 0x7fffffff, "am_head_post_f32: too many rows");
  HeadPostF32 p{X, ldx, off, head_stride, chunks, heads, w, eps, rope_cos, rope_sin, rope_cos ? rows_per_frame : 1};
  hipLaunchKernelGGL(head_post_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  AM_HIP(hipGetLastError());
  return AM_OK;
}

extern "C" int am_rope_f32(float* X, int64_t ldx, int off_a, int off_b, int head_stride, int64_t rows, int heads, const float* rope_cos,
                           const float* rope_sin, int frames, int rows_per_frame, void* stream) {
  AM_CHECK((rope_cos == nullptr) == (rope_sin == nullptr), "am_rope_f32: rope tables must come in pairs");
  AM_CHECK(X && rope_cos, "am_rope_f32: null operand");
  AM_CHECK(rows > 0 && heads > 0 && heads <= 65535, "am_rope_f32: bad shape rows=%lld heads=%d", (long long)rows, heads);
  const int kinds = off_b < 0 ? 1 : 2;
  AM_CHECK(al16(X) && heads_aligned(ldx, off_a, head_stride) && (kinds == 1 || heads_aligned(ldx, off_b, head_stride)),
           "am_rope_f32: X, ldx, off_a, off_b and head_stride must be 16-byte aligned");
  AM_CHECK((heads == 1 || head_stride >= HP_D) && heads_fit(ldx, off_a, head_stride, heads, HP_D) &&
               (kinds == 1 || heads_fit(ldx, off_b, head_stride, heads, HP_D)),
           "am_rope_f32: the heads' chunks overlap or run past the row (ldx=%lld off_a=%d off_b=%d head_stride=%d heads=%d)",
           (long long)ldx, off_a, off_b, head_stride, heads);
  if (kinds == 2) {
    // a q chunk and a k chunk overlap when off_b - off_a + m head_stride lies inside (-128, 128) for a head difference |m| < heads;
    // with head_stride >= 128 only the two multiples around the difference can
    const int64_t d = (int64_t)off_b - off_a;
    bool overlap;
    if (heads == 1) {
      overlap = d > -HP_D && d < HP_D;
    } else {
      const int64_t fl = d >= 0 ? d / head_stride : -((-d + head_stride - 1) / head_stride);      // floor(d / head_stride)
      const int64_t r = d - fl * head_stride;                                                     // in [0, head_stride)
      overlap = (r < HP_D && fl < heads && -fl < heads) || (head_stride - r < HP_D && fl + 1 < heads && -(fl + 1) < heads);
    }
    AM_CHECK(!overlap, "am_rope_f32: the q and k chunks overlap (off_a=%d off_b=%d head_stride=%d heads=%d)", off_a, off_b, head_stride, heads);
  }
  AM_CHECK(frames_cover(rows, rows_per_frame, frames),
           "am_rope_f32: rows=%lld / rows_per_frame=%d runs past the %d frames of the tables", (long long)rows, rows_per_frame, frames);
  const int64_t chunks = rows * heads * kinds, blocks = (chunks + HP_CHUNKS - 1) / HP_CHUNKS;
  AM_CHECK(blocks <= 0x7fffffff, "am_rope_f32: too many rows");
  RopeF32 p{X, ldx, {off_a, kinds == 2 ? off_b : off_a}, head_stride, chunks, heads, kinds, rope_cos, rope_sin, rows_per_frame};
  hipLaunchKernelGGL(rope_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  AM_HIP(hipGetLastError());
  return AM_OK;
}

extern "C" int am_flow_step_f32(const float* v_dev, float* latents_dev, int n_branches, const float* scales_host, float dt,
                                int is_additive, const uint8_t* unobserved_host, int T_local, int N, int Din, void* stream) {
  AM_CHECK(v_dev && latents_dev, "am_flow_step_f32: null operand");
  AM_CHECK(n_branches >= 1 && n_branches <= 4, "am_flow_step_f32: n_branches=%d", n_branches);
  AM_CHECK(n_branches == 1 || scales_host, "am_flow_step_f32: scales required");
  AM_CHECK(T_local > 0 && T_local <= 256 && N > 0 && Din > 0, "am_flow_step_f32: bad shape");
  FlowF32 a;
  a.v = v_dev;
  a.lat = latents_dev;
  a.nb = n_branches;
  for (int i = 0; i < 3; ++i) a.scales[i] = (i < n_branches - 1) ? scales_host[i] : 0.f;
  a.dt = dt;
  a.additive = is_additive ? 1 : 0;
  for (int f = 0; f < 256; ++f) a.unobs[f] = (f < T_local) ? (unobserved_host ? unobserved_host[f] : 1) : 0;
  const int64_t per_frame = (int64_t)N * Din;
  const bool vec = per_frame % 4 == 0 && al16(v_dev) && al16(latents_dev);
  a.per_frame4 = vec ? per_frame / 4 : per_frame;
  a.total4 = a.per_frame4 * T_local;
  const int64_t blocks = (a.total4 + 255) / 256;
  AM_CHECK(blocks <= 0x7fffffff, "am_flow_step_f32: too many elements");
  if (vec) hipLaunchKernelGGL(flow_step_f32_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(flow_step_f32_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  AM_HIP(hipGetLastError());
  return AM_OK;
}
