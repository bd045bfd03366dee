// Image preprocessing in front of the context encoder, bit-identical to the CPU code it replaces: the reference's ImagePreprocessor
// (actionmesh/preprocessing/image_processor.py:15-146) and the PIL backend of transformers' BitImageProcessor (image_encoder.py:48-51).
// The contract - validity, composite table, bounding box, padding, PIL's fixed-point bicubic resample, crop, normalisation table - is
// in include/actionmesh_amd.h; everything here is integer or table arithmetic, so there is nothing to round differently.
//
//   alpha statistics   grid (blocks, frames): 16-byte loads of four RGBA pixels, per-lane count / min / max, a wave reduction by
//                      shuffles, the workgroup's waves through LDS, then ONE integer atomic add / min / max per workgroup and value.
//   horizontal pass    grid (blocks, frames): a thread owns four adjacent output columns of one row of the padded image (12 bytes of
//                      the intermediate image: three 4-byte stores).  A source pixel is one 4-byte load (RGBA, then three lookups in
//                      the composite table) or two aligned 4-byte loads funnel-shifted (RGB).  The padded image is virtual.
//   vertical pass      a thread owns four adjacent columns of one output row: three 4-byte loads per tap row, then the uint8 crop
//                      (three 4-byte stores) and the fp32 pixel_values through the normalisation table (one 16-byte store per channel).
//   Tap tables of the columns / rows a crop needs are copied to LDS when they fit IMAGE_LDS_BYTES, and read from global memory beyond.
//   Every frame carries its own geometry (am_image_frame), so independently cropped frames share the launches.
#include "am_common.h"

#include <climits>

namespace {

constexpr int IMAGE_THREADS = 256;
constexpr int IMAGE_LDS_BYTES = 48 * 1024;      // most LDS a tap table may take; larger tables are read from global memory
constexpr int IMAGE_MAX_DIM = 1 << 20;          // pixels per side of a padded image (keeps every 32-bit product below 2^31 with the checks)

// ---- alpha statistics -----------------------------------------------------------------------------------------------------------
__global__ void image_stats_init_kernel(int32_t* __restrict__ stats, int n_frames) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_frames * 8) return;
  const int k = i & 7;
  stats[i] = (k == 1 || k == 2) ? INT_MAX : ((k == 3 || k == 4) ? -1 : 0);
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// `vec`: every frame starts 16-byte aligned and holds a multiple of four pixels.
__global__ __launch_bounds__(IMAGE_THREADS) void image_alpha_stats_kernel(const uint32_t* __restrict__ rgba, int npix, int width, int vec,
                                                                           int32_t* __restrict__ stats) {
  __shared__ int32_t part[IMAGE_THREADS / 64][5];
  const int t = blockIdx.y;
  const uint32_t* __restrict__ frame = rgba + (int64_t)t * npix;
  int cnt = 0, minx = INT_MAX, miny = INT_MAX, maxx = -1, maxy = -1;
  const int64_t step = (int64_t)gridDim.x * IMAGE_THREADS * 4;
  for (int64_t p = ((int64_t)blockIdx.x * IMAGE_THREADS + threadIdx.x) * 4; p < npix; p += step) {
    uint32_t v[4];
    if (vec) {
      const u32x4_t q = *reinterpret_cast<const u32x4_t*>(frame + p);
      v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = p + e < npix ? frame[p + e] : 0u;      // a pixel beyond the frame counts as alpha 0
    }
    int y = (int)(p / width), x = (int)(p - (int64_t)y * width);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t a = v[e] >> 24;
      cnt += a > 127u;
      if (a > 0u) {
        minx = min(minx, x); maxx = max(maxx, x);
        miny = min(miny, y); maxy = max(maxy, y);
      }
      if (++x == width) { x = 0; ++y; }
    }
  }
  cnt = wave_sum(cnt);
  minx = wave_min(minx); miny = wave_min(miny);
  maxx = wave_max(maxx); maxy = wave_max(maxy);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    part[wave][0] = cnt; part[wave][1] = minx; part[wave][2] = miny; part[wave][3] = maxx; part[wave][4] = maxy;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < IMAGE_THREADS / 64; ++w) {
      cnt += part[w][0];
      minx = min(minx, part[w][1]); miny = min(miny, part[w][2]);
      maxx = max(maxx, part[w][3]); maxy = max(maxy, part[w][4]);
    }
    int32_t* s = stats + t * 8;
    atomicAdd(s + 0, cnt);
    atomicMin(s + 1, minx); atomicMin(s + 2, miny);
    atomicMax(s + 3, maxx); atomicMax(s + 4, maxy);
  }
}

// ---- the virtual source image ---------------------------------------------------------------------------------------------------
struct ImageSrc {
  const uint8_t* src;
  int64_t src_bytes;
  const uint8_t* composite;
  int fill;
};

// Pixel (yv, xv) of frame f's padded image: the window of the stored frame inside pad_x / pad_y of `fill`.
template <int CH>
__device__ __forceinline__ void image_fetch(const ImageSrc& s, const am_image_frame& f, int yv, int xv, int (&c)[3]) {
  const int xs = xv - f.pad_x, ys = yv - f.pad_y;
  if ((unsigned)xs >= (unsigned)f.w || (unsigned)ys >= (unsigned)f.h) {
    c[0] = c[1] = c[2] = s.fill;
    return;
  }
  const int64_t p = (int64_t)(f.y0 + ys) * f.src_w + (f.x0 + xs);
  if constexpr (CH == 4) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(s.src + f.src_offset + p * 4);
    const uint32_t a = v >> 24;
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = s.composite[(((v >> (8 * k)) & 255u) << 8) + a];
  } else {
    const int64_t b = f.src_offset + p * 3, a0 = b & ~(int64_t)3;
    const int sh = (int)(b & 3);
    if (a0 + 8 <= s.src_bytes) {                // both words lie inside the buffer
      const uint32_t w0 = *reinterpret_cast<const uint32_t*>(s.src + a0);
      const uint32_t w1 = sh >= 2 ? *reinterpret_cast<const uint32_t*>(s.src + a0 + 4) : 0u;
      const uint32_t v = (uint32_t)((((uint64_t)w1 << 32) | w0) >> (8 * sh));
#pragma unroll
      for (int k = 0; k < 3; ++k) c[k] = (int)((v >> (8 * k)) & 255u);
    } else {                                    // the last bytes of the buffer
#pragma unroll
      for (int k = 0; k < 3; ++k) c[k] = s.src[b + k];
    }
  }
}

__device__ __forceinline__ uint32_t clip8(int v) {
  v >>= 22;                                     // arithmetic
  return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// The part of a tap table that `n` outputs starting at `first` need: their (first tap, count) pairs and coefficient rows, in LDS when
// `use_lds` (after a barrier every thread of the workgroup reaches), else where they are.
__device__ __forceinline__ void image_taps(const int32_t* __restrict__ tab, int first, int n, int use_lds, int32_t* lds,
                                           const int32_t*& bounds, const int32_t*& coef, int& ks) {
  const int out = tab[1];
  ks = tab[2];
  bounds = tab + 4 + 2 * first;
  coef = tab + 4 + 2 * (int64_t)out + (int64_t)first * ks;
  if (use_lds) {
    for (int i = threadIdx.x; i < 2 * n; i += IMAGE_THREADS) lds[i] = bounds[i];
    for (int i = threadIdx.x; i < n * ks; i += IMAGE_THREADS) lds[2 * n + i] = coef[i];
    __syncthreads();
    bounds = lds;
    coef = lds + 2 * n;
  }
}

// hbuf: (n_frames, max_rows, pitch) bytes, pitch = 12 * groups (four output columns of three channels per group)
template <int CH>
__global__ __launch_bounds__(IMAGE_THREADS) void image_hpass_kernel(ImageSrc s, const am_image_frame* __restrict__ frames,
                                                                     const int32_t* __restrict__ taps, int cw, int groups, int max_rows,
                                                                     int use_lds, uint8_t* __restrict__ hbuf) {
  extern __shared__ __attribute__((aligned(16))) int32_t image_lds[];
  const int t = blockIdx.y;
  const am_image_frame f = frames[t];
  const int32_t *bounds, *coef;
  int ks;
  image_taps(taps + f.htab, f.left, cw, use_lds, image_lds, bounds, coef, ks);
  const int64_t idx = (int64_t)blockIdx.x * IMAGE_THREADS + threadIdx.x;
  const int r = (int)(idx / groups), g = (int)(idx - (int64_t)r * groups);
  if (r >= f.n_rows) return;
  const int yv = f.row_lo + r;
  uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int col = 4 * g + e;
    if (col >= cw) break;
    const int x0 = bounds[2 * col], n = bounds[2 * col + 1];
    const int32_t* __restrict__ k = coef + (int64_t)col * ks;
    int acc[3] = {1 << 21, 1 << 21, 1 << 21};
    for (int j = 0; j < n; ++j) {
      int c[3];
      image_fetch<CH>(s, f, yv, x0 + j, c);
      const int kj = k[j];
      acc[0] += kj * c[0]; acc[1] += kj * c[1]; acc[2] += kj * c[2];
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int byte = 3 * e + ch;
      o[byte >> 2] |= clip8(acc[ch]) << (8 * (byte & 3));
    }
  }
  uint32_t* dst = reinterpret_cast<uint32_t*>(hbuf + ((int64_t)t * max_rows + r) * ((int64_t)groups * 12) + (int64_t)g * 12);
  dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
}

__global__ __launch_bounds__(IMAGE_THREADS) void image_vpass_kernel(const uint8_t* __restrict__ hbuf, const am_image_frame* __restrict__ frames,
                                                                     const int32_t* __restrict__ taps, int cw, int ch_out, int groups,
                                                                     int max_rows, int use_lds, const float* __restrict__ norm,
                                                                     float* __restrict__ out_pixels, uint8_t* __restrict__ out_u8) {
  extern __shared__ __attribute__((aligned(16))) int32_t image_lds[];
  const int t = blockIdx.y;
  const am_image_frame f = frames[t];
  const int32_t *bounds, *coef;
  int ks;
  image_taps(taps + f.vtab, f.top, ch_out, use_lds, image_lds, bounds, coef, ks);
  const int64_t idx = (int64_t)blockIdx.x * IMAGE_THREADS + threadIdx.x;
  const int i = (int)(idx / groups), g = (int)(idx - (int64_t)i * groups);
  if (i >= ch_out) return;
  const int y0 = bounds[2 * i] - f.row_lo, n = bounds[2 * i + 1];
  const int32_t* __restrict__ k = coef + (int64_t)i * ks;
  const int64_t pitch = (int64_t)groups * 12;
  const uint8_t* __restrict__ col0 = hbuf + ((int64_t)t * max_rows + y0) * pitch + (int64_t)g * 12;
  int acc[12];
#pragma unroll
  for (int b = 0; b < 12; ++b) acc[b] = 1 << 21;
  for (int j = 0; j < n; ++j) {
    const uint32_t* __restrict__ row = reinterpret_cast<const uint32_t*>(col0 + j * pitch);
    const uint32_t w0 = row[0], w1 = row[1], w2 = row[2];
    const int kj = k[j];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      acc[b] += kj * (int)((w0 >> (8 * b)) & 255u);
      acc[4 + b] += kj * (int)((w1 >> (8 * b)) & 255u);
      acc[8 + b] += kj * (int)((w2 >> (8 * b)) & 255u);
    }
  }
  uint32_t v[12];
#pragma unroll
  for (int b = 0; b < 12; ++b) v[b] = clip8(acc[b]);
  const int64_t row_px = ((int64_t)t * ch_out + i) * cw + 4 * g;                // first pixel of the group in the (T, ch, cw) image
  const bool full = (cw & 3) == 0;                                              // then every group is whole and every store aligned
  if (out_u8) {
    if (full) {
      uint32_t* dst = reinterpret_cast<uint32_t*>(out_u8 + row_px * 3);
#pragma unroll
      for (int w = 0; w < 3; ++w) dst[w] = v[4 * w] | (v[4 * w + 1] << 8) | (v[4 * w + 2] << 16) | (v[4 * w + 3] << 24);
    } else {
#pragma unroll
      for (int b = 0; b < 12; ++b)
        if (4 * g + b / 3 < cw) out_u8[row_px * 3 + b] = (uint8_t)v[b];
    }
  }
  if (out_pixels) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* dst = out_pixels + (((int64_t)t * 3 + c) * ch_out + i) * cw + 4 * g;
      const float* __restrict__ tb = norm + c * 256;
      if (full) {
        const f32x4_t q = {tb[v[c]], tb[v[3 + c]], tb[v[6 + c]], tb[v[9 + c]]};
        *reinterpret_cast<f32x4_t*>(dst) = q;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (4 * g + e < cw) dst[e] = tb[v[3 * e + c]];
      }
    }
  }
}

// The padded, composited frames themselves (ImagePreprocessor.process_images' output): four pixels = 12 bytes per thread.
template <int CH>
__global__ __launch_bounds__(IMAGE_THREADS) void image_materialize_kernel(ImageSrc s, const am_image_frame* __restrict__ frames,
                                                                           uint8_t* __restrict__ out) {
  const am_image_frame f = frames[blockIdx.y];
  const int wv = f.w + 2 * f.pad_x, hv = f.h + 2 * f.pad_y;
  const int64_t npix = (int64_t)wv * hv;
  const int64_t q = (int64_t)blockIdx.x * IMAGE_THREADS + threadIdx.x, p0 = q * 4;
  if (p0 >= npix) return;
  int y = (int)(p0 / wv), x = (int)(p0 - (int64_t)y * wv);
  uint32_t o[3] = {0u, 0u, 0u};
  uint8_t* dst = out + f.dst_offset + p0 * 3;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (p0 + e >= npix) break;
    int c[3];
    image_fetch<CH>(s, f, y, x, c);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int byte = 3 * e + ch;
      o[byte >> 2] |= (uint32_t)c[ch] << (8 * (byte & 3));
    }
    if (++x == wv) { x = 0; ++y; }
  }
  if (p0 + 4 <= npix) {
    uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
    d4[0] = o[0]; d4[1] = o[1]; d4[2] = o[2];
  } else {
    const int nb = (int)(npix - p0) * 3;
    for (int b = 0; b < nb; ++b) dst[b] = (uint8_t)(o[b >> 2] >> (8 * (b & 3)));
  }
}

// ---- host: validation -----------------------------------------------------------------------------------------------------------
int image_check_src(const char* who, const uint8_t* src, int64_t src_bytes, int channels, int fill, const uint8_t* composite, int n_frames,
                    const am_image_frame* frames, const am_image_frame* frames_dev) {
  AM_CHECK(n_frames >= 1 && n_frames <= 65535, "%s: n_frames %d outside 1 .. 65535", who, n_frames);
  AM_CHECK(channels == 3 || channels == 4, "%s: src_channels %d is not 3 (RGB) or 4 (RGBA)", who, channels);
  AM_CHECK(fill >= 0 && fill <= 255, "%s: fill %d outside 0 .. 255", who, fill);
  AM_CHECK(src != nullptr && src_bytes > 0, "%s: no source image", who);
  AM_CHECK((reinterpret_cast<uintptr_t>(src) & 3) == 0, "%s: src must be 4-byte aligned", who);
  AM_CHECK(channels == 3 || composite != nullptr, "%s: an RGBA source needs the composite table", who);
  AM_CHECK(frames != nullptr && frames_dev != nullptr, "%s: frames and frames_dev are both needed", who);
  for (int t = 0; t < n_frames; ++t) {
    const am_image_frame& f = frames[t];
    AM_CHECK(f.src_w >= 1 && f.src_h >= 1 && f.src_w <= IMAGE_MAX_DIM && f.src_h <= IMAGE_MAX_DIM, "%s: frame %d: stored size %d x %d", who, t,
             f.src_w, f.src_h);
    AM_CHECK(f.src_offset >= 0 && (f.src_offset & 3) == 0, "%s: frame %d: src_offset %lld is negative or not a multiple of 4", who, t,
             (long long)f.src_offset);
    AM_CHECK(f.src_offset + (int64_t)f.src_w * f.src_h * channels <= src_bytes, "%s: frame %d: %d x %d x %d bytes at %lld exceed src_bytes %lld",
             who, t, f.src_h, f.src_w, channels, (long long)f.src_offset, (long long)src_bytes);
    AM_CHECK(f.x0 >= 0 && f.y0 >= 0 && f.w >= 1 && f.h >= 1 && f.x0 <= f.src_w - f.w && f.y0 <= f.src_h - f.h,
             "%s: frame %d: window (%d, %d, %d, %d) outside the stored %d x %d", who, t, f.x0, f.y0, f.w, f.h, f.src_w, f.src_h);
    AM_CHECK(f.pad_x >= 0 && f.pad_y >= 0 && f.pad_x <= IMAGE_MAX_DIM && f.pad_y <= IMAGE_MAX_DIM &&
                 (int64_t)f.w + 2 * (int64_t)f.pad_x <= IMAGE_MAX_DIM && (int64_t)f.h + 2 * (int64_t)f.pad_y <= IMAGE_MAX_DIM,
             "%s: frame %d: padding (%d, %d) is negative or the padded image exceeds %d pixels a side", who, t, f.pad_x, f.pad_y, IMAGE_MAX_DIM);
  }
  return AM_OK;
}

// One tap table against the image it samples: header, extent, and - for the `n` outputs from `first` - every tap inside [lo, hi).
int image_check_table(int t, const char* axis, const int32_t* taps, int64_t taps_len, int32_t off, int in, int first, int n, int lo, int hi,
                      int* ksize) {
  AM_CHECK(off >= 0 && (int64_t)off + 4 <= taps_len, "am_image_resample: frame %d: %s table offset %d outside taps (%lld)", t, axis, off,
           (long long)taps_len);
  const int32_t* tab = taps + off;
  const int out = tab[1], ks = tab[2];
  AM_CHECK(tab[0] == in, "am_image_resample: frame %d: %s table is for %d input samples, the padded image has %d", t, axis, tab[0], in);
  AM_CHECK(out >= 1 && out <= IMAGE_MAX_DIM && ks >= 1 && ks <= IMAGE_MAX_DIM, "am_image_resample: frame %d: %s table header (out %d, ksize %d)",
           t, axis, out, ks);
  AM_CHECK((int64_t)off + 4 + 2 * (int64_t)out + (int64_t)out * ks <= taps_len, "am_image_resample: frame %d: %s table runs past taps_len", t, axis);
  AM_CHECK(first >= 0 && n >= 1 && first <= out - n, "am_image_resample: frame %d: %s crop [%d, %d + %d) outside the resized %d", t, axis, first,
           first, n, out);
  for (int i = first; i < first + n; ++i) {
    const int a = tab[4 + 2 * i], c = tab[4 + 2 * i + 1];
    AM_CHECK(c >= 0 && c <= ks && a >= lo && a <= hi - c, "am_image_resample: frame %d: %s output %d reads taps [%d, %d + %d) outside [%d, %d)", t,
             axis, i, a, a, c, lo, hi);
  }
  *ksize = ks;
  return AM_OK;
}

int image_groups(int out_w) { return (out_w + 3) / 4; }

}  // namespace

extern "C" int am_image_alpha_stats(const am_image_alpha_stats_args* a, void* stream) {
  AM_CHECK(a != nullptr, "am_image_alpha_stats: null arguments");
  AM_CHECK(a->rgba != nullptr && a->out_stats != nullptr, "am_image_alpha_stats: null pointer");
  AM_CHECK((reinterpret_cast<uintptr_t>(a->rgba) & 3) == 0, "am_image_alpha_stats: rgba must be 4-byte aligned");
  AM_CHECK(a->n_frames >= 1 && a->n_frames <= 65535, "am_image_alpha_stats: n_frames %d outside 1 .. 65535", a->n_frames);
  AM_CHECK(a->height >= 1 && a->width >= 1 && (int64_t)a->height * a->width < ((int64_t)1 << 31), "am_image_alpha_stats: frame size %d x %d",
           a->height, a->width);
  hipStream_t st = (hipStream_t)stream;
  const int npix = a->height * a->width;
  const int vec = (npix & 3) == 0 && (reinterpret_cast<uintptr_t>(a->rgba) & 15) == 0;
  hipLaunchKernelGGL(image_stats_init_kernel, dim3(ceil_div((int64_t)a->n_frames * 8, IMAGE_THREADS)), dim3(IMAGE_THREADS), 0, st, a->out_stats,
                     a->n_frames);
  int blocks = ceil_div(npix, IMAGE_THREADS * 4 * 4);          // four 16-byte loads per thread
  blocks = blocks < 1 ? 1 : (blocks > 256 ? 256 : blocks);
  hipLaunchKernelGGL(image_alpha_stats_kernel, dim3(blocks, a->n_frames), dim3(IMAGE_THREADS), 0, st,
                     reinterpret_cast<const uint32_t*>(a->rgba), npix, a->width, vec, a->out_stats);
  AM_HIP(hipGetLastError());
  return AM_OK;
}

extern "C" size_t am_image_resample_workspace_bytes(int n_frames, int max_rows, int out_w) {
  if (n_frames < 1 || max_rows < 1 || out_w < 1) return 0;
  return (size_t)n_frames * (size_t)max_rows * (size_t)image_groups(out_w) * 12;
}

extern "C" int am_image_resample(const am_image_resample_args* a, void* stream) {
  AM_CHECK(a != nullptr, "am_image_resample: null arguments");
  AM_TRY(image_check_src("am_image_resample", a->src, a->src_bytes, a->src_channels, a->fill, a->composite, a->n_frames, a->frames, a->frames_dev));
  AM_CHECK(a->out_w >= 1 && a->out_h >= 1 && a->out_w <= IMAGE_MAX_DIM && a->out_h <= IMAGE_MAX_DIM, "am_image_resample: output size %d x %d",
           a->out_w, a->out_h);
  AM_CHECK(a->taps != nullptr && a->taps_dev != nullptr && a->taps_len >= 4, "am_image_resample: taps and taps_dev are both needed");
  AM_CHECK(a->out_pixels != nullptr || a->out_u8 != nullptr, "am_image_resample: neither out_pixels nor out_u8 is given");
  AM_CHECK(a->out_pixels == nullptr || a->norm_table != nullptr, "am_image_resample: out_pixels needs norm_table");
  AM_CHECK((reinterpret_cast<uintptr_t>(a->out_pixels) & 15) == 0 && (reinterpret_cast<uintptr_t>(a->out_u8) & 3) == 0,
           "am_image_resample: out_pixels must be 16-byte and out_u8 4-byte aligned");
  int max_rows = 0, ks_h = 0, ks_v = 0;
  for (int t = 0; t < a->n_frames; ++t) {
    const am_image_frame& f = a->frames[t];
    const int in_w = f.w + 2 * f.pad_x, in_h = f.h + 2 * f.pad_y;
    AM_CHECK(f.row_lo >= 0 && f.n_rows >= 1 && f.row_lo <= in_h - f.n_rows, "am_image_resample: frame %d: rows [%d, %d + %d) outside the padded %d",
             t, f.row_lo, f.row_lo, f.n_rows, in_h);
    int kh = 0, kv = 0;
    AM_TRY(image_check_table(t, "horizontal", a->taps, a->taps_len, f.htab, in_w, f.left, a->out_w, 0, in_w, &kh));
    AM_TRY(image_check_table(t, "vertical", a->taps, a->taps_len, f.vtab, in_h, f.top, a->out_h, f.row_lo, f.row_lo + f.n_rows, &kv));
    max_rows = f.n_rows > max_rows ? f.n_rows : max_rows;
    ks_h = kh > ks_h ? kh : ks_h;
    ks_v = kv > ks_v ? kv : ks_v;
  }
  const size_t need = am_image_resample_workspace_bytes(a->n_frames, max_rows, a->out_w);
  AM_CHECK(a->workspace != nullptr && a->workspace_bytes >= need, "am_image_resample: workspace of %zu bytes needed, %zu given", need,
           (size_t)a->workspace_bytes);
  AM_CHECK((reinterpret_cast<uintptr_t>(a->workspace) & 15) == 0, "am_image_resample: the workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int groups = image_groups(a->out_w);
  const ImageSrc s = {a->src, a->src_bytes, a->composite, a->fill};
  uint8_t* hbuf = reinterpret_cast<uint8_t*>(a->workspace);
  const int64_t lds_h = (int64_t)a->out_w * (2 + ks_h) * 4, lds_v = (int64_t)a->out_h * (2 + ks_v) * 4;
  const int use_h = lds_h <= IMAGE_LDS_BYTES, use_v = lds_v <= IMAGE_LDS_BYTES;
  const int64_t bh = ((int64_t)max_rows * groups + IMAGE_THREADS - 1) / IMAGE_THREADS, bv = ((int64_t)a->out_h * groups + IMAGE_THREADS - 1) / IMAGE_THREADS;
  AM_CHECK(bh < ((int64_t)1 << 31) && bv < ((int64_t)1 << 31), "am_image_resample: the problem exceeds one launch grid");
  const dim3 gh((unsigned)bh, a->n_frames), gv((unsigned)bv, a->n_frames);
  if (a->src_channels == 4)
    hipLaunchKernelGGL(image_hpass_kernel<4>, gh, dim3(IMAGE_THREADS), use_h ? (size_t)lds_h : 0, st, s, a->frames_dev, a->taps_dev, a->out_w, groups,
                       max_rows, use_h, hbuf);
  else
    hipLaunchKernelGGL(image_hpass_kernel<3>, gh, dim3(IMAGE_THREADS), use_h ? (size_t)lds_h : 0, st, s, a->frames_dev, a->taps_dev, a->out_w, groups,
                       max_rows, use_h, hbuf);
  hipLaunchKernelGGL(image_vpass_kernel, gv, dim3(IMAGE_THREADS), use_v ? (size_t)lds_v : 0, st, hbuf, a->frames_dev, a->taps_dev, a->out_w, a->out_h,
                     groups, max_rows, use_v, a->norm_table, a->out_pixels, a->out_u8);
  AM_HIP(hipGetLastError());
  return AM_OK;
}

extern "C" int am_image_materialize(const am_image_materialize_args* a, void* stream) {
  AM_CHECK(a != nullptr, "am_image_materialize: null arguments");
  AM_TRY(image_check_src("am_image_materialize", a->src, a->src_bytes, a->src_channels, a->fill, a->composite, a->n_frames, a->frames, a->frames_dev));
  AM_CHECK(a->out != nullptr && (reinterpret_cast<uintptr_t>(a->out) & 3) == 0, "am_image_materialize: out must be a 4-byte aligned device pointer");
  int64_t max_pix = 0;
  for (int t = 0; t < a->n_frames; ++t) {
    const am_image_frame& f = a->frames[t];
    const int64_t npix = (int64_t)(f.w + 2 * f.pad_x) * (f.h + 2 * f.pad_y);
    AM_CHECK(f.dst_offset >= 0 && (f.dst_offset & 3) == 0 && f.dst_offset + npix * 3 <= a->out_bytes,
             "am_image_materialize: frame %d: %lld bytes at dst_offset %lld do not fit out_bytes %lld (or the offset is not a multiple of 4)", t,
             (long long)(npix * 3), (long long)f.dst_offset, (long long)a->out_bytes);
    max_pix = npix > max_pix ? npix : max_pix;
  }
  const int64_t blocks = ((max_pix + 3) / 4 + IMAGE_THREADS - 1) / IMAGE_THREADS;
  AM_CHECK(blocks < ((int64_t)1 << 31), "am_image_materialize: the problem exceeds one launch grid");
  const ImageSrc s = {a->src, a->src_bytes, a->composite, a->fill};
  hipStream_t st = (hipStream_t)stream;
  if (a->src_channels == 4)
    hipLaunchKernelGGL(image_materialize_kernel<4>, dim3((unsigned)blocks, a->n_frames), dim3(IMAGE_THREADS), 0, st, s, a->frames_dev, a->out);
  else
    hipLaunchKernelGGL(image_materialize_kernel<3>, dim3((unsigned)blocks, a->n_frames), dim3(IMAGE_THREADS), 0, st, s, a->frames_dev, a->out);
  AM_HIP(hipGetLastError());
  return AM_OK;
}
