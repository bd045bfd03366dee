// Farthest-point sampling: the point-cloud reduction in front of the TripoSG VAE (reference actionmesh/external/triposg.py:113-151
// through actionmesh/model/utils/pointcloud_sampling.py, which calls pytorch3d.ops.sample_farthest_points on CUDA).  Exact greedy
// FPS as include/actionmesh_amd.h states it: K strictly sequential steps, so what counts is the latency of ONE step.
//
//   grid = batch: one workgroup per cloud, no communication between workgroups (and so no grid-wide barrier).
//   Resident form (n_points <= FPS_RESIDENT): lane t owns the points j * THREADS + t.  Their first dist_dims channels (as fp32) and
//   their running minimum distance md stay in REGISTERS for the whole launch: global memory is read once, and written K indices.
//   One step:
//     per lane   d2 / md update of its PPT points and the lane's (largest md, lowest j), the coordinates of that point carried
//                along by conditional moves (no dynamically indexed register array, so nothing goes to scratch);
//     per wave   two 32-bit DPP reductions: the largest md (its bit pattern as an unsigned number: md >= 0, so the bits order),
//                then the lowest point index among the lanes that hold it;
//     workgroup  the wave's owner lane writes (md, index, coordinates) to the wave's LDS slot; ONE __syncthreads (the slots are
//                double-buffered by step parity, so the next step's writes cannot overtake this step's reads); every wave then
//                reduces the slots the same way and reads the winner's coordinates from its slot - not from HBM.
//   The distance channels are zero-padded to 3 or 8: a padding channel adds (0 - 0)^2 = +0 to a non-negative sum, which changes
//   no bit, so two instantiations cover dist_dims 1..8.
//   Streaming form (n_points > FPS_RESIDENT): the same workgroup; md and a channel-major fp32 copy of the distance channels live in a
//   caller-supplied workspace (L2-resident for any realistic size) and are walked with 16-byte loads every step - the caller's
//   array-of-points layout costs a wave six cache lines per 4-byte load, which is what bounded the first version of this form;
//   the winner's coordinates are one uniform global read.
//   d2 = ((d0*d0) + (d1*d1)) + (d2*d2) + ... with contraction OFF: every product and sum rounded on its own.
//   Non-finite inputs: md = fmin(md, d2) drops a NaN d2, so md stays in [0, +inf] and every index stays inside [0, n_points).
#include "am_common.h"

namespace {

constexpr int FPS_RESIDENT = 8192;        // most points the resident form holds (THREADS * PPT of every full-size instantiation)
constexpr int FPS_SMALL = 2048;           // the short-cloud instantiations (a quarter of the per-lane work)
constexpr int FPS_STREAM_THREADS = 1024;
constexpr int FPS_DEFAULT_THREADS = 512;
constexpr uint32_t INF_BITS = 0x7f800000u;

__device__ __forceinline__ float fps_load(const void* p, int64_t off, int dtype) {
  if (dtype == AM_FPS_F32) return reinterpret_cast<const float*>(p)[off];
  const uint16_t h = reinterpret_cast<const uint16_t*>(p)[off];
  if (dtype == AM_FPS_F16) return (float)__builtin_bit_cast(_Float16, h);
  return __builtin_bit_cast(float, (uint32_t)h << 16);
}

// DPP controls (gfx9): row_shr:n = 0x110 + n, row_bcast:15 = 0x142, row_bcast:31 = 0x143.  A lane without a source gets `old`,
// the operation's identity (which also lets the compiler fold the move into v_max_u32_dpp / v_min_u32_dpp).  After the four shifts lane 15 of every 16-lane row holds the row's result;
// bcast:15 folds row 0 into row 1 and row 2 into row 3, bcast:31 folds lane 31 into rows 2-3: lane 63 holds the wave's.
// Needs all 64 lanes active: only ever called from workgroup-uniform control flow.
#define FPS_DPP(v, id, ctrl, rows) (uint32_t)__builtin_amdgcn_update_dpp((int)(id), (int)(v), ctrl, rows, 0xf, false)
__device__ __forceinline__ uint32_t wave_umax(uint32_t v) {
  v = max(v, FPS_DPP(v, 0u, 0x111, 0xf));
  v = max(v, FPS_DPP(v, 0u, 0x112, 0xf));
  v = max(v, FPS_DPP(v, 0u, 0x114, 0xf));
  v = max(v, FPS_DPP(v, 0u, 0x118, 0xf));
  v = max(v, FPS_DPP(v, 0u, 0x142, 0xa));
  v = max(v, FPS_DPP(v, 0u, 0x143, 0xc));
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint32_t wave_umin(uint32_t v) {
  v = min(v, FPS_DPP(v, 0xffffffffu, 0x111, 0xf));
  v = min(v, FPS_DPP(v, 0xffffffffu, 0x112, 0xf));
  v = min(v, FPS_DPP(v, 0xffffffffu, 0x114, 0xf));
  v = min(v, FPS_DPP(v, 0xffffffffu, 0x118, 0xf));
  v = min(v, FPS_DPP(v, 0xffffffffu, 0x142, 0xa));
  v = min(v, FPS_DPP(v, 0xffffffffu, 0x143, 0xc));
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// One wave's LDS slot: what its best point looks like to the rest of the workgroup.
template <int DD> struct FpsSlot { uint32_t bits, idx; float c[DD]; };

// (largest md, lowest index) over the workgroup.  In: each lane's candidate (bits = md's bit pattern, idx, and - when DD > 0 - its
// coordinates).  Out, identical in every thread: the winner.  `slots` is the buffer of this step's parity.  Exactly one
// __syncthreads, reached by every thread.
template <int THREADS, int DD>
__device__ __forceinline__ void block_argmax(uint32_t& bits, uint32_t& idx, float (&c)[DD > 0 ? DD : 1],
                                             FpsSlot<(DD > 0 ? DD : 1)>* slots) {
  constexpr int W = THREADS / 64;
  static_assert(W >= 1 && W <= 64, "one lane per wave slot");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t wmax = wave_umax(bits);
  const uint32_t widx = wave_umin(bits == wmax ? idx : 0xffffffffu);
  if (idx == widx && bits == wmax) {            // indices are unique: one lane per wave
    slots[wave].bits = wmax;
    slots[wave].idx = widx;
#pragma unroll
    for (int d = 0; d < DD; ++d) slots[wave].c[d] = c[d];
  }
  __syncthreads();
  const uint32_t sb = lane < W ? slots[lane].bits : 0u;
  const uint32_t si = lane < W ? slots[lane].idx : 0xffffffffu;
  bits = wave_umax(sb);
  idx = wave_umin(sb == bits ? si : 0xffffffffu);
  const int owner = (int)(idx & (uint32_t)(THREADS - 1)) >> 6;      // idx = j * THREADS + t: the wave of thread t
#pragma unroll
  for (int d = 0; d < DD; ++d) c[d] = slots[owner].c[d];
}

template <int THREADS, int PPT, int DD>
__global__ __launch_bounds__(THREADS) void fps_resident_kernel(const void* __restrict__ points, int dtype, int n, int dist_dims,
                                                               int64_t batch_stride, int64_t point_stride, int n_samples,
                                                               const int32_t* __restrict__ start_idx, int32_t* __restrict__ out_index,
                                                               float* __restrict__ out_dist) {
#pragma clang fp contract(off)
  __shared__ FpsSlot<DD> slots[2][THREADS / 64];
  const int b = blockIdx.x, t = threadIdx.x;
  const int64_t base = (int64_t)b * batch_stride;
  float p[PPT][DD], md[PPT];
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int i = j * THREADS + t;
    const bool valid = i < n;
    md[j] = valid ? __builtin_bit_cast(float, INF_BITS) : 0.f;      // a padding slot: md 0 and an index above every real one - never the winner
#pragma unroll
    for (int d = 0; d < DD; ++d) p[j][d] = (valid && d < dist_dims) ? fps_load(points, base + (int64_t)i * point_stride + d, dtype) : 0.f;
  }
  int s = start_idx ? start_idx[b] : 0;
  s = s < 0 ? 0 : (s >= n ? n - 1 : s);
  uint32_t cur = (uint32_t)s, cur_bits = INF_BITS;
  float c[DD];
#pragma unroll
  for (int d = 0; d < DD; ++d) c[d] = d < dist_dims ? fps_load(points, base + (int64_t)s * point_stride + d, dtype) : 0.f;
  out_index += (int64_t)b * n_samples;
  if (out_dist) out_dist += (int64_t)b * n_samples;
  for (int k = 0;; ++k) {
    if (t == 0) {
      out_index[k] = (int32_t)cur;
      if (out_dist) out_dist[k] = __builtin_bit_cast(float, cur_bits);
    }
    if (k == n_samples - 1) break;              // uniform: the last sample needs no further update
    float best = -1.f;
    int bj = 0;
    float bc[DD];
#pragma unroll
    for (int d = 0; d < DD; ++d) bc[d] = 0.f;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      float d0 = p[j][0] - c[0];
      float acc = d0 * d0;
#pragma unroll
      for (int d = 1; d < DD; ++d) {
        const float dd = p[j][d] - c[d];
        const float sq = dd * dd;
        acc = acc + sq;
      }
      md[j] = __builtin_fminf(md[j], acc);
      const bool better = md[j] > best;         // strict, j ascending: the lane's lowest index among equals
      best = better ? md[j] : best;
      bj = better ? j : bj;
#pragma unroll
      for (int d = 0; d < DD; ++d) bc[d] = better ? p[j][d] : bc[d];
    }
    cur_bits = __builtin_bit_cast(uint32_t, best);
    cur = (uint32_t)(bj * THREADS + t);
    block_argmax<THREADS, DD>(cur_bits, cur, bc, slots[k & 1]);
#pragma unroll
    for (int d = 0; d < DD; ++d) c[d] = bc[d];
  }
}

// DD as in the resident form (zero-padded channels).  Workspace of one cloud: md[npad], then channel d of every point at
// ch[d * npad + i] (npad = n rounded up to 4): thread t owns the points 4 * (t + T * trip) .. + 3 of every trip, so a wave's load is
// one contiguous KiB, and a thread only ever reads workspace words it wrote itself (no ordering between threads is needed).
// U trips are in flight together.
template <int DD, int U>
__global__ __launch_bounds__(FPS_STREAM_THREADS) void fps_stream_kernel(const void* __restrict__ points, int dtype, int64_t n, int dist_dims,
                                                                        int64_t batch_stride, int64_t point_stride, int n_samples,
                                                                        const int32_t* __restrict__ start_idx,
                                                                        int32_t* __restrict__ out_index, float* __restrict__ out_dist,
                                                                        float* __restrict__ ws) {
#pragma clang fp contract(off)
  constexpr int T = FPS_STREAM_THREADS;
  __shared__ FpsSlot<1> slots[2][T / 64];
  const int b = blockIdx.x, t = threadIdx.x;
  const int64_t base = (int64_t)b * batch_stride;
  const int64_t npad = (n + 3) & ~(int64_t)3;
  float* __restrict__ md = ws + (int64_t)b * npad * (1 + dist_dims);
  float* __restrict__ ch = md + npad;
  const f32x4_t inf4 = {__builtin_bit_cast(float, INF_BITS), __builtin_bit_cast(float, INF_BITS), __builtin_bit_cast(float, INF_BITS),
                        __builtin_bit_cast(float, INF_BITS)};
  const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
  // once: the distance channels as fp32, channel-major
  for (int64_t i = (int64_t)t * 4; i < n; i += (int64_t)T * 4) {
#pragma unroll
    for (int d = 0; d < DD; ++d) {
      if (d < dist_dims) {
        f32x4_t v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = i + e < n ? fps_load(points, base + (i + e) * point_stride + d, dtype) : 0.f;
        *reinterpret_cast<f32x4_t*>(ch + d * npad + i) = v;
      }
    }
  }
  int64_t s = start_idx ? start_idx[b] : 0;
  s = s < 0 ? 0 : (s >= n ? n - 1 : s);
  uint32_t cur = (uint32_t)s, cur_bits = INF_BITS;
  out_index += (int64_t)b * n_samples;
  if (out_dist) out_dist += (int64_t)b * n_samples;
  for (int k = 0;; ++k) {
    if (t == 0) {
      out_index[k] = (int32_t)cur;
      if (out_dist) out_dist[k] = __builtin_bit_cast(float, cur_bits);
    }
    if (k == n_samples - 1) break;
    float c[DD];        // from the caller's array, not the workspace copy another thread wrote
#pragma unroll
    for (int d = 0; d < DD; ++d) c[d] = d < dist_dims ? fps_load(points, base + (int64_t)cur * point_stride + d, dtype) : 0.f;
    float best = -1.f;
    uint32_t bi = 0;
    // ascending indices within the thread, so the strict compare keeps its lowest one
    for (int64_t i0 = (int64_t)t * 4; i0 < n; i0 += (int64_t)T * 4 * U) {
      f32x4_t x[U][DD], old[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t i = i0 + (int64_t)u * T * 4;
        const bool valid = i < n;               // then i + 3 < npad
        old[u] = (valid && k > 0) ? *reinterpret_cast<const f32x4_t*>(md + i) : inf4;
#pragma unroll
        for (int d = 0; d < DD; ++d) x[u][d] = (valid && d < dist_dims) ? *reinterpret_cast<const f32x4_t*>(ch + d * npad + i) : zero4;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t i = i0 + (int64_t)u * T * 4;
        if (i < n) {
          f32x4_t m4;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float d0 = x[u][0][e] - c[0];
            float acc = d0 * d0;
#pragma unroll
            for (int d = 1; d < DD; ++d) {
              const float dd = x[u][d][e] - c[d];
              const float sq = dd * dd;
              acc = acc + sq;
            }
            const float m = __builtin_fminf(old[u][e], acc);
            m4[e] = m;
            if (i + e < n && m > best) {        // the padding points of the last group of four never compete
              best = m;
              bi = (uint32_t)(i + e);
            }
          }
          *reinterpret_cast<f32x4_t*>(md + i) = m4;
        }
      }
    }
    cur_bits = __builtin_bit_cast(uint32_t, best < 0.f ? 0.f : best);      // a thread without a point (never, for n > FPS_RESIDENT) must not win
    cur = bi;
    float none[1] = {0.f};
    block_argmax<T, 0>(cur_bits, cur, none, slots[k & 1]);
  }
}

template <int DD, int U>
void fps_launch_stream(const am_fps_args* a, hipStream_t st) {
  hipLaunchKernelGGL((fps_stream_kernel<DD, U>), dim3(a->batch), dim3(FPS_STREAM_THREADS), 0, st, a->points, a->dtype, a->n_points,
                     a->dist_dims, a->batch_stride, a->point_stride, (int)a->n_samples, a->start_idx, a->out_index, a->out_dist,
                     reinterpret_cast<float*>(a->workspace));
}

int fps_check(const am_fps_args* a) {
  AM_CHECK(a != nullptr, "am_fps: null arguments");
  AM_CHECK(a->dtype == AM_FPS_F32 || a->dtype == AM_FPS_F16 || a->dtype == AM_FPS_BF16, "am_fps: unknown dtype %d", a->dtype);
  AM_CHECK(a->batch >= 1 && a->n_points >= 1, "am_fps: empty problem (batch %d, %lld points)", a->batch, (long long)a->n_points);
  AM_CHECK(a->n_points < (int64_t)1 << 31, "am_fps: %lld points do not fit a 32-bit index", (long long)a->n_points);
  AM_CHECK(a->n_samples >= 1 && a->n_samples <= a->n_points, "am_fps: n_samples %lld outside 1 .. n_points (%lld)",
           (long long)a->n_samples, (long long)a->n_points);
  AM_CHECK(a->dims >= 1 && a->dims <= 8, "am_fps: dims %d outside 1 .. 8", a->dims);
  AM_CHECK(a->dist_dims >= 1 && a->dist_dims <= a->dims, "am_fps: dist_dims %d outside 1 .. dims (%d)", a->dist_dims, a->dims);
  AM_CHECK(a->point_stride >= a->dims, "am_fps: point_stride %lld is less than dims (%d)", (long long)a->point_stride, a->dims);
  AM_CHECK(a->batch_stride >= 0, "am_fps: negative batch_stride %lld", (long long)a->batch_stride);
  AM_CHECK(a->threads == 0 || a->threads == 256 || a->threads == 512 || a->threads == 1024, "am_fps: threads %d is not 0, 256, 512 or 1024",
           a->threads);
  AM_CHECK(a->points && a->out_index, "am_fps: null pointer");
  const size_t need = am_fps_workspace_bytes(a->n_points, a->batch, a->dist_dims);
  AM_CHECK(need == 0 || (a->workspace != nullptr && a->workspace_bytes >= need), "am_fps: workspace of %zu bytes needed, %zu given", need,
           (size_t)a->workspace_bytes);
  AM_CHECK(need == 0 || (reinterpret_cast<uintptr_t>(a->workspace) & 15) == 0, "am_fps: the workspace must be 16-byte aligned");
  return AM_OK;
}

template <int THREADS, int PPT, int DD>
void fps_launch_resident(const am_fps_args* a, hipStream_t st) {
  hipLaunchKernelGGL((fps_resident_kernel<THREADS, PPT, DD>), dim3(a->batch), dim3(THREADS), 0, st, a->points, a->dtype, (int)a->n_points,
                     a->dist_dims, a->batch_stride, a->point_stride, (int)a->n_samples, a->start_idx, a->out_index, a->out_dist);
}

template <int DD>
void fps_dispatch_resident(const am_fps_args* a, int threads, hipStream_t st) {
  const bool small = a->n_points <= FPS_SMALL;
  if constexpr (DD <= 3) {                      // 32 points x 8 channels would not fit one wave's registers: wide clouds start at 512
    if (threads == 256) {
      if (small) fps_launch_resident<256, FPS_SMALL / 256, DD>(a, st);
      else fps_launch_resident<256, FPS_RESIDENT / 256, DD>(a, st);
      return;
    }
  }
  if (threads == 1024) {
    if (small) fps_launch_resident<1024, FPS_SMALL / 1024, DD>(a, st);
    else fps_launch_resident<1024, FPS_RESIDENT / 1024, DD>(a, st);
  } else {
    if (small) fps_launch_resident<512, FPS_SMALL / 512, DD>(a, st);
    else fps_launch_resident<512, FPS_RESIDENT / 512, DD>(a, st);
  }
}

}  // namespace

extern "C" size_t am_fps_workspace_bytes(int64_t n_points, int batch, int dist_dims) {
  if (n_points <= FPS_RESIDENT || batch < 1 || dist_dims < 1 || dist_dims > 8) return 0;
  const size_t npad = ((size_t)n_points + 3) & ~(size_t)3;
  return sizeof(float) * (size_t)batch * npad * (size_t)(1 + dist_dims);       // md + the distance channels as fp32, channel-major
}

extern "C" int am_fps(const am_fps_args* a, void* stream) {
  AM_TRY(fps_check(a));
  hipStream_t st = (hipStream_t)stream;
  if (a->n_points > FPS_RESIDENT) {
    if (a->dist_dims <= 3) fps_launch_stream<3, 2>(a, st);
    else fps_launch_stream<8, 2>(a, st);
  } else {
    const int threads = a->threads ? a->threads : FPS_DEFAULT_THREADS;
    if (a->dist_dims <= 3) fps_dispatch_resident<3>(a, threads, st);
    else fps_dispatch_resident<8>(a, threads, st);
  }
  AM_HIP(hipGetLastError());
  return AM_OK;
}
