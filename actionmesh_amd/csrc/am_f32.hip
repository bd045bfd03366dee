// Exact-fp32 matrix path (gfx950 v_mfma_f32_32x32x2_f32: fp32 operands, fp32 accumulation, bitwise a k-ordered fmaf chain).
// What the reference runs with autocast off - Stage II's query side and cross-attention block (temporal_autoencoder.py:240-243,
// 266-267) and the DINOv2 context encoder (pipeline.py:665-667) - runs here in fp32:
//   am_gemm_f32        C = A W^T (+ bias) (GELU) (+ R), R may alias C                       (nn.Linear in fp32)
//   am_attention_f32   non-causal SDPA, head_dim 64 / 128, operands read in place from packed projection outputs
//   am_layernorm_f32   nn.LayerNorm in fp32
//   am_displacement_f32: the fp32-input form of am_displacement (am_point_embed_f32 / am_patchify_f32 are in am_elementwise.hip,
//   next to the 16-bit forms they share their kernels with).
// Deterministic: no split-K, no atomics; every launch of the same shape computes the same bits (both library builds compile this
// file the same way - nothing in it depends on the 16-bit type).  Built without the SLP vectoriser (csrc/Makefile).
#include <math.h>

#include "am_common.h"

namespace {

__device__ __forceinline__ f32x16_t mfma_f32(float a, float b, f32x16_t c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
// row of element r of a 32x32 accumulator held by lane half h (the column is the lane index & 31)
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// ---- GEMM ---------------------------------------------------------------------------------------------------------------------
// 128 x 128 output tile per workgroup (4 waves, 2 x 2 of 64 x 64, each 2 x 2 MFMA tiles of 32 x 32), K in slices of 32.
// Operand fragment of k-step s (0..15) for lane half h: X[row = lane & 31][k = 16 h + s] - both A (rows m) and W (rows n, the B
// operand B[k][n] = W[n][k]) are read that way, so a lane reads 16 consecutive k of one row (four ds_read_b128).  The slice walks
// k in the order (s, h); the sum is the same fmaf chain for every launch.  LDS: [row][32 + 4] (conflict-free b128 reads),
// double-buffered through registers: one barrier per slice.
constexpr int GT = 128, GK = 32, GLD = GK + 4;
constexpr int G_SMEM = 2 * 2 * GT * GLD * 4;   // [buffer][A | W][row][GLD] floats: 73 728 bytes

struct GemmF32 {
  const float* A; const float* W; const float* bias; const float* R; float* C;
  int64_t lda, ldw, ldr, ldc;
  int M, N, K, act;
};

__global__ __launch_bounds__(256, 2) void gemm_f32_kernel(GemmF32 p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* lds = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, c = lane & 31;
  const int m0 = blockIdx.y * GT, n0 = blockIdx.x * GT;
  const int wm = (wave & 1) * 64, wn = (wave >> 1) * 64;
  const int kq = tid & 7, lrow = tid >> 3;          // loader: 8 float4 per 32-float row slice, rows lrow + 32 i
  const int nk = (p.K + GK - 1) / GK;

  f32x4_t ra[4], rw[4];
  auto load = [&](int t) {
    const int k = t * GK + kq * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + lrow + 32 * i, n = n0 + lrow + 32 * i;
      ra[i] = (m < p.M && k < p.K) ? *reinterpret_cast<const f32x4_t*>(p.A + (int64_t)m * p.lda + k) : f32x4_t{0.f, 0.f, 0.f, 0.f};
      rw[i] = (n < p.N && k < p.K) ? *reinterpret_cast<const f32x4_t*>(p.W + (int64_t)n * p.ldw + k) : f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto store = [&](int buf) {
    float* la = lds + buf * 2 * GT * GLD;
    float* lw = la + GT * GLD;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<f32x4_t*>(la + (lrow + 32 * i) * GLD + kq * 4) = ra[i];
      *reinterpret_cast<f32x4_t*>(lw + (lrow + 32 * i) * GLD + kq * 4) = rw[i];
    }
  };

  f32x16_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  load(0);
  store(0);
  __syncthreads();
  for (int t = 0; t < nk; ++t) {
    if (t + 1 < nk) load(t + 1);
    const float* la = lds + (t & 1) * 2 * GT * GLD;
    const float* lw = la + GT * GLD;
#pragma unroll
    for (int q = 0; q < 4; ++q) {               // four k-steps per b128 read
      f32x4_t a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = *reinterpret_cast<const f32x4_t*>(la + (wm + 32 * i + c) * GLD + 16 * h + 4 * q);
        b[i] = *reinterpret_cast<const f32x4_t*>(lw + (wn + 32 * i + c) * GLD + 16 * h + 4 * q);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = mfma_f32(a[i][e], b[j][e], acc[i][j]);
    }
    if (t + 1 < nk) store((t + 1) & 1);
    __syncthreads();
  }

  // epilogue: element r of acc[i][j] is C[m0 + wm + 32 i + acc_row(r, h)][n0 + wn + 32 j + c]; R is read before C is written by
  // the same lane, so R may alias C
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + wn + 32 * j + c;
    if (n >= p.N) continue;
    const float bn = p.bias ? p.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm + 32 * i + acc_row(r, h);
        if (m >= p.M) continue;
        float v = acc[i][j][r] + bn;
        if (p.act == 1) v = v * 0.5f * (1.0f + erff(v * 0.70710678118654752440f));   // F.gelu(approximate="none")
        if (p.R) v += p.R[(int64_t)m * p.ldr + n];
        p.C[(int64_t)m * p.ldc + n] = v;
      }
  }
}

// ---- attention ----------------------------------------------------------------------------------------------------------------
// One workgroup = 4 waves = 128 query rows of one (sequence, head); each wave owns 32 queries, lane & 31 is its query.
// Per block of 32 keys:
//   S^T = K Q^T  on MFMA (A = K [key][d], B = Q^T, d walked as 64 h + s): element r of the accumulator is the score of key
//        acc_row(r, h) for the lane's own query, so a row's max / sum is 16 registers plus one exchange with lane ^ 32;
//   exact online softmax on ms = max scaled score: ms' = max(ms, block max * scale), p = expf(s scale - ms'), O and l rescaled by
//        expf(ms - ms');
//   O^T = O^T alpha + V^T P^T, the block product on MFMA: the probabilities are the B operand as they lie (k-step s = key
//        acc_row(s, h)), V^T the A operand.
// K / V tiles go through LDS ([key][D + 4] / [key][D + 8]: conflict-free reads), double-buffered through registers.
struct AttnF32 {
  const float* Q; const float* K; const float* V; float* O;
  int64_t ldq, ldk, ldv, ldo;
  int q_off, q_hs, k_off, k_hs, v_off, v_hs;
  int nseq, heads, sq, sk;
  float scale;
};
constexpr int AQ = 128, AK = 32;
template <int D> struct AttnGeo {
  static constexpr int KLD = D + 4, VLD = D + 8;
  static constexpr int BUF = AK * (KLD + VLD);                 // floats per buffer
  static constexpr int SMEM = 2 * BUF * 4;
  static constexpr int PER = AK * D / 4 / 256;                 // float4 per thread per operand per block
};

template <int D>
__global__ __launch_bounds__(256, D == 128 ? 1 : 2) void attention_f32_kernel(AttnF32 p) {
  using G = AttnGeo<D>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* lds = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, c = lane & 31;
  const int seq = blockIdx.z, head = blockIdx.y;
  const int qi = blockIdx.x * AQ + wave * 32 + c;
  const int64_t qrow = (int64_t)seq * p.sq + qi;

  float qf[D / 2];                                  // Q[qi][D/2 h + s]
  if (qi < p.sq) {
    const float* qp = p.Q + qrow * p.ldq + p.q_off + (int64_t)head * p.q_hs + (D / 2) * h;
#pragma unroll
    for (int s = 0; s < D / 2; s += 4) {
      const f32x4_t v = *reinterpret_cast<const f32x4_t*>(qp + s);
#pragma unroll
      for (int e = 0; e < 4; ++e) qf[s + e] = v[e];
    }
  } else {
#pragma unroll
    for (int s = 0; s < D / 2; ++s) qf[s] = 0.f;
  }

  const float* kbase = p.K + (int64_t)seq * p.sk * p.ldk + p.k_off + (int64_t)head * p.k_hs;
  const float* vbase = p.V + (int64_t)seq * p.sk * p.ldv + p.v_off + (int64_t)head * p.v_hs;
  // next block's K is loaded before the scores and stored behind them, its V loaded behind the scores and stored behind P.V: the two
  // register stages are never live together
  f32x4_t rk[G::PER], rv[G::PER];
  auto load = [&](const float* base, int64_t ld, int kb, f32x4_t* r) {
#pragma unroll
    for (int i = 0; i < G::PER; ++i) {
      const int idx = tid + 256 * i, key = idx / (D / 4), dq = idx % (D / 4);
      const int kk = kb * AK + key;
      r[i] = kk < p.sk ? *reinterpret_cast<const f32x4_t*>(base + (int64_t)kk * ld + 4 * dq) : f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto store = [&](float* dst, int ld, const f32x4_t* r) {
#pragma unroll
    for (int i = 0; i < G::PER; ++i) {
      const int idx = tid + 256 * i, key = idx / (D / 4), dq = idx % (D / 4);
      *reinterpret_cast<f32x4_t*>(dst + key * ld + 4 * dq) = r[i];
    }
  };

  f32x16_t o[D / 32];
#pragma unroll
  for (int t = 0; t < D / 32; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
  float ms = -INFINITY, l = 0.f;                    // running max of the SCALED scores (rounded once), running sum

  const int nkb = (p.sk + AK - 1) / AK;
  load(kbase, p.ldk, 0, rk);
  load(vbase, p.ldv, 0, rv);
  store(lds, G::KLD, rk);
  store(lds + AK * G::KLD, G::VLD, rv);
  __syncthreads();
  for (int kb = 0; kb < nkb; ++kb) {
    const bool more = kb + 1 < nkb;
    if (more) load(kbase, p.ldk, kb + 1, rk);
    const float* ks = lds + (kb & 1) * G::BUF;
    const float* vs = ks + AK * G::KLD;
    float* nks = lds + ((kb + 1) & 1) * G::BUF;
    f32x16_t sacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
    for (int s = 0; s < D / 2; s += 4) {
      const f32x4_t a = *reinterpret_cast<const f32x4_t*>(ks + c * G::KLD + (D / 2) * h + s);
#pragma unroll
      for (int e = 0; e < 4; ++e) sacc = mfma_f32(a[e], qf[s + e], sacc);
      if (s % 16 == 12) __builtin_amdgcn_sched_barrier(0);    // keeps the scheduler from hoisting every K read (D = 128 spilled)
    }
    if (more) {
      store(nks, G::KLD, rk);
      load(vbase, p.ldv, kb + 1, rv);
    }
    // mask the keys past sk (last block only), block max of the lane's query
    const int kvalid = p.sk - kb * AK;
    float bm = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (acc_row(r, h) >= kvalid) sacc[r] = -INFINITY;
      bm = fmaxf(bm, sacc[r]);
    }
    bm = fmaxf(bm, __shfl_xor(bm, 32));
    // every exponent is taken against the same rounded ms the rescale uses: alpha is exactly 1 while the max stands (an unrounded
    // m * scale in the rescale drifted the early blocks' weight by (1 + ulp(ms))^blocks: 2.9e-6 rel-L2 at sk = 4113, D = 128)
    const float msn = fmaxf(ms, bm * p.scale);
    const float alpha = expf(ms - msn);                    // ms = -inf on the first block: 0
    float bs = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      sacc[r] = expf(fmaf(sacc[r], p.scale, -msn));
      bs += sacc[r];
    }
    bs += __shfl_xor(bs, 32);
    l = fmaf(l, alpha, bs);
    ms = msn;
    // each block's P.V starts from zero and is folded in as o = o alpha + block (the same one VALU op per element the rescale costs):
    // a 32-key partial sum per fmaf chain instead of one chain over all sk keys.  With a near-uniform softmax over zero-mean V the
    // result is ~sqrt(sk) smaller than sum |p v|, and the single chain's rounding grew as eps sqrt(sk / 2) relative to it (measured
    // 3.2e-6 rel-L2 at sk = 4113, D = 128); blocked, it is ~eps (sqrt(16) + sqrt(sk / 64)).
#pragma unroll
    for (int t = 0; t < D / 32; ++t) {
      f32x16_t blk;
#pragma unroll
      for (int r = 0; r < 16; ++r) blk[r] = 0.f;
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        blk = mfma_f32(vs[acc_row(s, h) * G::VLD + 32 * t + c], sacc[s], blk);
        if (s == 7) __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) o[t][r] = fmaf(o[t][r], alpha, blk[r]);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (more) store(nks + AK * G::KLD, G::VLD, rv);
    __syncthreads();
  }

  // element r of o[t] is O[qi][32 t + acc_row(r, h)]: registers 4g .. 4g + 3 are four consecutive columns
  if (qi < p.sq) {
    float* op = p.O + qrow * p.ldo + (int64_t)head * D;
#pragma unroll
    for (int t = 0; t < D / 32; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<f32x4_t*>(op + 32 * t + 8 * g + 4 * h) =
            f32x4_t{o[t][4 * g] / l, o[t][4 * g + 1] / l, o[t][4 * g + 2] / l, o[t][4 * g + 3] / l};
  }
}

// ---- LayerNorm (fp32 in / out), one wave per row, two-pass statistics ------------------------------------------------------------
template <int NCH>
__global__ __launch_bounds__(256) void layernorm_f32_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ w,
                                                            const float* __restrict__ b, int64_t rows, int C, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + row * C;
  f32x4_t v[NCH];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int col = (j * 64 + lane) * 4;
    v[j] = col < C ? *reinterpret_cast<const f32x4_t*>(xr + col) : f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) sum += v[j][e];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
  const float mean = sum / (float)C;
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int col = (j * 64 + lane) * 4;
    if (col < C) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = v[j][e] - mean;
        sq += d * d;
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off);
  const float rstd = 1.0f / sqrtf(sq / (float)C + eps);
  float* yr = y + row * C;
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int col = (j * 64 + lane) * 4;
    if (col < C) {
      const f32x4_t wv = *reinterpret_cast<const f32x4_t*>(w + col), bv = *reinterpret_cast<const f32x4_t*>(b + col);
      f32x4_t o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (v[j][e] - mean) * rstd * wv[e] + bv[e];
      *reinterpret_cast<f32x4_t*>(yr + col) = o;
    }
  }
}

// temporal_autoencoder.py:156-157, 267 on fp32 logits: 2 sigmoid(-logits) - 1, libm expf
__global__ void displacement_f32_kernel(const float* __restrict__ logits, int ld, int64_t rows, int out_dim, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * out_dim) return;
  const int64_t row = i / out_dim;
  out[i] = 2.0f / (1.0f + expf(logits[row * ld + (i - row * out_dim)])) - 1.0f;
}

}  // namespace

extern "C" int am_gemm_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias, const float* R, int64_t ldr,
                           float* C, int64_t ldc, int M, int N, int K, int act, void* stream) {
  AM_CHECK(A && W && C, "am_gemm_f32: null operand");
  AM_CHECK(M > 0 && N > 0 && K > 0 && K % 4 == 0, "am_gemm_f32: bad shape M=%d N=%d K=%d (K %% 4 == 0)", M, N, K);
  AM_CHECK(act == 0 || act == 1, "am_gemm_f32: act=%d (0 none, 1 erf-GELU)", act);
  AM_CHECK(lda >= K && ldw >= K && lda % 4 == 0 && ldw % 4 == 0 && al16(A) && al16(W),
           "am_gemm_f32: A / W need 16-byte aligned rows (lda=%lld ldw=%lld)", (long long)lda, (long long)ldw);
  AM_CHECK(ldc >= N && (!R || ldr >= N), "am_gemm_f32: ldc=%lld / ldr=%lld < N=%d", (long long)ldc, (long long)ldr, N);
  AM_ONCE_PER_DEVICE({
    AM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_f32_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, G_SMEM));
  });
  GemmF32 p{A, W, bias, R, C, lda, ldw, R ? ldr : 0, ldc, M, N, K, act};
  hipLaunchKernelGGL(gemm_f32_kernel, dim3(ceil_div(N, GT), ceil_div(M, GT)), dim3(256), G_SMEM, (hipStream_t)stream, p);
  AM_HIP(hipGetLastError());
  return AM_OK;
}

extern "C" int am_attention_f32(const am_attn_f32_args* a, void* stream) {
  AM_CHECK(a && a->Q && a->K && a->V && a->O, "am_attention_f32: null operand");
  const int D = a->head_dim;
  AM_CHECK(D == 64 || D == 128, "am_attention_f32: head_dim %d (64 or 128)", D);
  AM_CHECK(a->nseq > 0 && a->heads > 0 && a->sq > 0 && a->sk > 0 && a->nseq <= 65535 && a->heads <= 65535,
           "am_attention_f32: bad shape nseq=%d heads=%d sq=%d sk=%d", a->nseq, a->heads, a->sq, a->sk);
  AM_CHECK(al16(a->Q) && al16(a->K) && al16(a->V) && al16(a->O) && (a->ldo & 3) == 0 && heads_aligned(a->ldq, a->q_off, a->q_hs) &&
           heads_aligned(a->ldk, a->k_off, a->k_hs) && heads_aligned(a->ldv, a->v_off, a->v_hs),
           "am_attention_f32: operands, row strides, column offsets and head strides must be 16-byte aligned");
  AM_CHECK(a->q_hs >= 0 && a->k_hs >= 0 && a->v_hs >= 0 && heads_fit(a->ldq, a->q_off, a->q_hs, a->heads, D) &&
           heads_fit(a->ldk, a->k_off, a->k_hs, a->heads, D) && heads_fit(a->ldv, a->v_off, a->v_hs, a->heads, D) &&
           a->ldo >= (int64_t)a->heads * D,
           "am_attention_f32: a head's columns run past its row (ld / offset / head stride)");
  AttnF32 p{a->Q, a->K, a->V, a->O, a->ldq, a->ldk, a->ldv, a->ldo, a->q_off, a->q_hs, a->k_off, a->k_hs, a->v_off, a->v_hs,
            a->nseq, a->heads, a->sq, a->sk, a->scale};
  const dim3 grid(ceil_div(a->sq, AQ), a->heads, a->nseq), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (D == 128) {
    AM_ONCE_PER_DEVICE({
      AM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(attention_f32_kernel<128>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 AttnGeo<128>::SMEM));
    });
    hipLaunchKernelGGL(attention_f32_kernel<128>, grid, block, AttnGeo<128>::SMEM, s, p);
  } else {
    hipLaunchKernelGGL(attention_f32_kernel<64>, grid, block, AttnGeo<64>::SMEM, s, p);
  }
  AM_HIP(hipGetLastError());
  return AM_OK;
}

extern "C" int am_layernorm_f32(const float* x, float* y, const float* w, const float* b, int64_t rows, int C, float eps, void* stream) {
  AM_CHECK(x && y && w && b, "am_layernorm_f32: null operand");
  AM_CHECK(rows > 0 && C > 0 && C % 4 == 0 && C <= 4096, "am_layernorm_f32: bad shape rows=%lld C=%d", (long long)rows, C);
  AM_CHECK(al16(x) && al16(y) && al16(w) && al16(b), "am_layernorm_f32: operands misaligned");
  const dim3 grid(ceil_div(rows, 4)), block(256);
  const int nch = ceil_div(C, 256);
  hipStream_t s = (hipStream_t)stream;
  if (nch <= 1) hipLaunchKernelGGL(layernorm_f32_kernel<1>, grid, block, 0, s, x, y, w, b, rows, C, eps);
  else if (nch <= 2) hipLaunchKernelGGL(layernorm_f32_kernel<2>, grid, block, 0, s, x, y, w, b, rows, C, eps);
  else if (nch <= 4) hipLaunchKernelGGL(layernorm_f32_kernel<4>, grid, block, 0, s, x, y, w, b, rows, C, eps);
  else if (nch <= 8) hipLaunchKernelGGL(layernorm_f32_kernel<8>, grid, block, 0, s, x, y, w, b, rows, C, eps);
  else hipLaunchKernelGGL(layernorm_f32_kernel<16>, grid, block, 0, s, x, y, w, b, rows, C, eps);
  AM_HIP(hipGetLastError());
  return AM_OK;
}

extern "C" int am_displacement_f32(const float* logits, int ld, int64_t rows, int out_dim, float* out, void* stream) {
  AM_CHECK(logits && out && rows > 0 && out_dim > 0 && ld >= out_dim, "am_displacement_f32: bad args");
  const int64_t n = rows * out_dim;
  hipLaunchKernelGGL(displacement_f32_kernel, dim3((unsigned)ceil_div(n, (int64_t)256)), dim3(256), 0, (hipStream_t)stream, logits, ld,
                     rows, out_dim, out);
  AM_HIP(hipGetLastError());
  return AM_OK;
}
