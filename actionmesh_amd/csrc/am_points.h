// What the point searches share (am_pointcloud.hip: brute force, am_nn_grid.hip: the grid, am_icp.hip: the fused ICP iteration): the
// arithmetic that makes their (index, d2) results the same bits - the squared distance, which candidate wins, the scan of a cloud
// staged through LDS - and the size checks of their entry points.  Everything sits in the unnamed namespace, next to the kernels of
// the source that includes it.
#pragma once
#include "am_common.h"

#pragma clang fp contract(off)      // the helpers below too, whatever flags the file is built with

namespace {

constexpr int NN_THREADS = 256;     // the workgroup of a staged scan
constexpr int NN_TILE = 512;        // points staged per pass

template <typename T> struct Vec4 { T x, y, z, w; };      // a staged point {x, y, z, 0} in the compute type

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// d2 = ((dx*dx) + (dy*dy)) + dz*dz, every operation rounded on its own: the summation of cKDTree and of the numpy oracles
template <typename T>
__device__ __forceinline__ T dist2(T qx, T qy, T qz, T px, T py, T pz) {
  const T dx = qx - px, dy = qy - py, dz = qz - pz;
  return (dx * dx + dy * dy) + dz * dz;
}

// Which candidate wins.  Both rules rest on two facts: a NaN or +inf distance never wins (no comparison with it is true against
// the initial +inf), and among equal distances the lowest index wins.  take_ascending is for candidates that arrive in ascending
// index order (a scan of the cloud; the splits of nn_reduce_kernel): the first minimum stays.  take_any_order is for any order
// (the grid's cells).
template <typename T>
__device__ __forceinline__ void take_ascending(T& best, int32_t& best_index, T d2, int32_t index) {
  if (d2 < best) best = d2, best_index = index;
}
template <typename T>
__device__ __forceinline__ void take_any_order(T& best, int32_t& best_index, T d2, int32_t index) {
  if (d2 < best || (d2 == best && index < best_index)) best = d2, best_index = index;
}

// The staged scan, called by all NN_THREADS threads of a workgroup: points lo .. hi - 1 of `src` pass through `tile` NN_TILE at a
// time, each staged once as stage(x, y, z) (in place, fp32) converted to T - the conversion is paid per tile, not per pair -, and
// every lane reads the same record (LDS broadcast) against its QPT queries (qx[j], qy[j], qz[j]), held in registers.
template <typename T, int QPT, typename Stage>
__device__ __forceinline__ void scan_staged(const float* __restrict__ src, int64_t lo, int64_t hi, Stage stage, Vec4<T> (&tile)[NN_TILE],
                                            const T (&qx)[QPT], const T (&qy)[QPT], const T (&qz)[QPT], T (&best)[QPT], int32_t (&bi)[QPT]) {
  for (int64_t base = lo; base < hi; base += NN_TILE) {
    const int n = (int)(hi - base < NN_TILE ? hi - base : NN_TILE);
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += NN_THREADS) {
      const float* s = src + (base + i) * 3;
      float x = s[0], y = s[1], z = s[2];
      stage(x, y, z);
      tile[i] = Vec4<T>{(T)x, (T)y, (T)z, (T)0};
    }
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < n; ++i) {
      const Vec4<T> p = tile[i];
#pragma unroll
      for (int j = 0; j < QPT; ++j) take_ascending(best[j], bi[j], dist2(qx[j], qy[j], qz[j], p.x, p.y, p.z), (int32_t)(base + i));
    }
  }
}
struct StageAsIs {
  __device__ __forceinline__ void operator()(float&, float&, float&) const {}
};

// the sizes every entry point checks first, in its own name: a batch of clouds of n `what` each, indexed in 32 bits, the batch on
// the launch grid's `axis` (0: it is not a grid axis)
bool cloud_ok(int batch, int64_t n) { return batch >= 1 && n >= 1 && n < (int64_t)1 << 31; }
int check_cloud(const char* who, int batch, int64_t n, const char* what, char axis) {
  AM_CHECK(batch >= 1 && n >= 1, "%s: empty problem (batch %d, %lld %s)", who, batch, (long long)n, what);
  AM_CHECK(n < (int64_t)1 << 31, "%s: %lld %s do not fit a 32-bit index", who, (long long)n, what);
  AM_CHECK(!axis || batch <= 65535, "%s: batch %d exceeds the grid's %c extent", who, batch, axis);
  return AM_OK;
}
// the workspace the caller passed against the size the entry point's own query returns.  Only am_nn_search has sizes that need
// none (one split): the ICP's and the grid build's need is never 0 once their sizes are valid, so a null workspace is refused there
int check_workspace(const char* who, const void* ws, size_t given, size_t need) {
  AM_CHECK(need == 0 || (ws != nullptr && given >= need), "%s: workspace of %zu bytes needed, %zu given", who, need, given);
  return AM_OK;
}

}  // namespace
