/*
 * actionmesh_amd.h - C ABI of libactionmesh_amd.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for ONE hot path of facebookresearch/actionmesh: the Stage-I
 * temporal-3D flow-matching denoise loop.  The reference has no FFI (it is pure
 * Python); its plug-in seams for this path are:
 *
 *   S1  actionmesh/scheduler/scheduler.py:252-295   SchedulerFlow.denoise
 *   S2  actionmesh/model/temporal_denoiser.py:151-249 ActionMeshDenoiser.forward
 *   S3  actionmesh/model/utils/attention_processor.py:36-168 AttentionProcessor.__call__
 *
 * Each entry point below names the reference interface it replaces.  The
 * reference-side binding (a ctypes stub) is shown in INTEGRATION.md; the
 * in-tree binding is actionmesh_amd/_lib.py.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch types.
 *   - every `*_dev` pointer is device memory valid on `stream` (a hipStream_t
 *     passed as void*; NULL = the null stream).  Pointers are borrowed for the
 *     duration of the call; nothing synchronises the device unless stated.
 *   - bf16 tensors are raw uint16 payloads, row-major.
 *   - return 0 on success, negative am_status otherwise; am_last_error() gives
 *     the message of the calling thread's last failure.
 *   - one handle per device per rank; a handle is not thread-safe (the
 *     reference drives this path from a single Python thread).
 */
#ifndef ACTIONMESH_AMD_H
#define ACTIONMESH_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  AM_OK = 0,
  AM_ERR_INVALID = -1,   /* bad argument / shape */
  AM_ERR_HIP = -2,       /* a HIP runtime call failed */
  AM_ERR_STATE = -3,     /* call sequence violated (e.g. forward before weights) */
  AM_ERR_NOTFOUND = -4   /* unknown weight name */
} am_status;

const char* am_last_error(void);
/* ABI version of this header; bumped on any signature change. */
int am_abi_version(void);

/* ------------------------------------------------------------------------ */
/* Model-level API                                                            */
/* ------------------------------------------------------------------------ */

/* Hyper-parameters of ActionMeshDenoiser (temporal_denoiser.py:29-48) plus the
 * static problem bounds the workspace is sized for. head_dim must be 128. */
typedef struct {
  int32_t in_channels;          /* Din (64) */
  int32_t num_layers;           /* NL (21) */
  int32_t num_heads;            /* H */
  int32_t width;                /* C = H*128 */
  int32_t ff_inner;             /* F = int(C*mlp_ratio) */
  int32_t cross_dim;            /* Dc (1024) */
  uint32_t inflated_mask_lo;    /* bit i set => layer i uses inflated (joint T*L) self-attention */
  uint32_t inflated_mask_hi;    /* layers 32..63 */
  int32_t max_batch;            /* CFG batch B (2) */
  int32_t max_frames_local;     /* frames owned by this rank (T / world) */
  int32_t max_tokens;           /* N latent tokens per frame */
  int32_t max_ctx_tokens;       /* S context tokens per frame */
  int32_t world_size;           /* frame-shard degree P (1 = single GPU) */
  int32_t rank;                 /* this rank's shard index */
  int32_t attn_defer_log2;      /* online-softmax deferred-rescale threshold (log2 units); 0 = always rescale */
  int32_t attn_fp8;             /* 1 = inflated self-attention on the fp8 kernel (am_attention_fp8); 0 = bf16 (default); 2 = fp8 with the
                                   exponent-field form of the probabilities (no v_exp: p = 2^n (1 + f), am_attention_fp8 defer_log2 = 5400) */
  int32_t reserved[6];
} am_config;

typedef struct am_model* am_handle;

int am_create(const am_config* cfg, am_handle* out);
int am_destroy(am_handle h);

/* Replaces PyTorchModelHubMixin.from_pretrained / load_state_dict for
 * ActionMeshDenoiser (pipeline.py:180-184).  `name` is a reference state-dict
 * key; `host_f32` is the fp32 tensor, row-major, `numel`
 * elements.  The library converts / fuses (q|k|v concatenated) and owns its copy. */
int am_load_weight(am_handle h, const char* name, const float* host_f32, size_t numel);
/* Number of reference state-dict keys still missing (0 = ready). */
int am_weights_missing(am_handle h);

/* Step-invariant conditioning for one window (replaces the per-step
 * to_k/to_v(context) of attention_processor.py:102-103 with a cache; and
 * precompute_freqs_rot, temporal_denoiser.py:114-149).
 *   ctx_dev       fp32 (B, T_local, S, Dc) device
 *   rope_cos/sin  fp32 host (B*T_local, 64): cos/sin of position*inv_freq per frame
 */
int am_set_context(am_handle h, const float* ctx_dev, int B, int T_local, int S,
                   const float* rope_cos_host, const float* rope_sin_host, void* stream);

/* Optional, after am_set_context: two EXACT shortcuts of the CFG batch (bit-identical results; the algorithmic flop count
 * of am_step_flops is unchanged and is what the bench reports against).  Cleared by the next am_set_context.
 *   ctx_is_zero_host[b] != 0: the context of batch row b is identically zero (the unconditional guidance branch,
 *       guidance.py:38-93).  to_k / to_v have no bias, so K = V = 0 and the cross-attention output of that row is exactly
 *       to_out[0].bias: the row's cross-attention branch (norm_x_attn, to_q, head split, SDPA, to_out) is
 *       replaced by h += bias, and its K/V cache is not built.  NULL = no row is zero.
 *   shared_prefix != 0: the caller asserts that every batch row carries the same hidden_states and the same t_bt (the sampler
 *       expands ONE latent tensor over the guidance branches, scheduler.py:215-217).  The rows then differ only from the first
 *       cross-attention on, so layer 0's skip-free prefix (norm_s_attn, QKV, qk-norm, RoPE, self-attention, to_out + residual)
 *       is computed for row 0 and copied to the other rows.  Ignored when world_size > 1. */
int am_set_branch_hints(am_handle h, const uint8_t* ctx_is_zero_host, int shared_prefix);

/* ActionMeshDenoiser.forward (temporal_denoiser.py:151-249), CFG-batched.
 *   x_dev     fp32 (B, T_local, N, Din)
 *   t_bt_host fp32 (B*T_local): per-(b,t) diffusion time AFTER the mask
 *             (temporal_denoiser.py:209-212)
 *   v_out_dev bf16 (B, T_local, N, Din)
 * Single-rank convenience = begin + for each layer {pre, post} + end. */
int am_denoise_forward(am_handle h, const float* x_dev, const float* t_bt_host,
                       int B, int T_local, int N, uint16_t* v_out_dev, void* stream);

/* am_denoise_forward through a HIP graph: the forward's ~450 launches are captured once per (x_dev, v_out_dev, shape, stream,
 * bound window) and replayed; the per-frame times are uploaded in front of every launch.  First call with a new key runs eagerly,
 * the second captures, later ones replay; a failed capture turns the path off for the handle (eager from then on).  The caller
 * keeps x_dev / v_out_dev at fixed addresses to benefit; `stream` must not be the null stream (falls back to eager).
 * am_graph_stats: counts4 = {replays, captures, eager forwards, capture failed}. */
int am_denoise_forward_graph(am_handle h, const float* x_dev, const float* t_bt_host,
                             int B, int T_local, int N, uint16_t* v_out_dev, void* stream);
int am_graph_stats(am_handle h, uint64_t* counts4);

/* The same forward, split at the temporal-attention boundary so the host can
 * run the K/V all-gather (RCCL) between `pre` and `post` of an inflated layer. */
int am_forward_begin(am_handle h, const float* x_dev, const float* t_bt_host,
                     int B, int T_local, int N, void* stream);
int am_layer_pre_attn(am_handle h, int layer, void* stream);   /* skip+LN+QKV+qk-norm+RoPE -> local K/V shard */
int am_layer_post_attn(am_handle h, int layer, void* stream);  /* self-attn .. FFN */
int am_forward_end(am_handle h, uint16_t* v_out_dev, void* stream);
/* Optional, multi-GPU: between pre_attn and post_attn of a layer, while the K/V all-gather is in flight, attend to
 * the LOCAL shard only (two-pass self-attention, am_attn_args.state_mode); post_attn then resumes over the remote
 * shards.  A no-op when the layer or the shapes do not qualify. */
int am_layer_attn_local(am_handle h, int layer, void* stream);

/* K / V^T gather buffers for inflated self-attention, laid out
 * [world][B][H][sk_pad][128] (K) and [world][B][H][128][sk_pad] (V^T); this
 * rank writes chunk `rank`.  By default the library owns them; a multi-GPU
 * host binds its own (torch-allocated) buffers so it can all-gather in place.
 * `chunk_stride_elems` = distance between consecutive ranks' chunks (0 = elems_per_chunk, i.e. two dense
 * arrays); 2 * elems_per_chunk with vt_dev = k_dev + elems_per_chunk interleaves [rank][K | V^T] so that ONE
 * all-gather per layer moves both operands. */
int am_kv_chunk_elems(am_handle h, size_t* elems_per_chunk);
int am_bind_kv_buffers(am_handle h, uint16_t* k_dev, uint16_t* vt_dev, size_t chunk_stride_elems);

/* fp8 handles (am_config.attn_fp8) with world_size > 1 exchange the QUANTISED shards: am_layer_pre_attn quantises this rank's K / V^T
 * shard into chunk `rank` of these buffers ([world][B][H][sk_pad][128] / [world][B][H][128][sk_pad] bytes; one byte per element,
 * chunk stride in bytes, 0 = elems_per_chunk), the host all-gathers them (half the bytes of the bf16 exchange), and the fp8
 * two-pass attention of am_layer_attn_local / am_layer_post_attn reads them.  Must be bound before the first forward; binding the
 * bf16 buffers on such a handle is an error.  With world_size = 1 the library owns its fp8 copies. */
int am_bind_kv8_buffers(am_handle h, uint8_t* k8_dev, uint8_t* vt8_dev, size_t chunk_stride_bytes);
/* counts2 = {fp8, bf16} inflated self-attention launches of the handle so far (a two-pass layer counts once). */
int am_attention_counters(am_handle h, uint64_t* counts2);

/* ClassifierFreeGuidance.aggregate_cfg (guidance.py:95-118) + the Euler flow
 * step and masked write of SchedulerFlow._flow_sample (scheduler.py:238-248):
 *   v = v_0 + sum_i scale_i (v_{i+1} - v_i)   (bf16 arithmetic, as the reference)
 *   latents[f] += sign * bf16(dt * v[f])  for frames with unobserved[f] != 0
 *   latents_dev fp32 (T_local, N, Din); v_dev bf16 (n_branches, T_local, N, Din) */
int am_flow_step(const uint16_t* v_dev, float* latents_dev, int n_branches,
                 const float* scales_host, float dt, int is_additive,
                 const uint8_t* unobserved_host, int T_local, int N, int Din, void* stream);

/* algorithmic flops of one forward (SURVEY.md 8(d) formula) for the bound shape */
double am_step_flops(am_handle h, int B, int T_total, int N, int S);

/* ------------------------------------------------------------------------ */
/* Kernel-level API (stateless).  These are what seam S3 binds, and what the   */
/* parity tests call one by one.                                               */
/* ------------------------------------------------------------------------ */

/* C[M,N] = act(A[M,K] @ W[N,K]^T + bias) + residual, bf16 in/out, fp32 accumulate.
 * Replaces nn.Linear (+ GELU of diffusers FeedForward, + the block's residual add)
 * at block.py:131-152 / attention_processor.py:92-103,147.
 *   A may be split in two column blocks (A1: first K1 cols, A2: rest) = the
 *   torch.cat([skip, h]) of block.py:131 without materialising it.
 *   Row maps: physical_row(r) = (r / G) * gs + off + r % G  (G = 0 => identity).
 *   residual uses C's row map and leading dimension; may alias C.
 *   Layout: A1, A2, W, C, residual 16-byte aligned; lda1, lda2, ldw, ldc multiples of 8
 *   elements; K and K1 multiples of 64, N a multiple of 8.  bias: 16-byte aligned on the
 *   256x256 tile (N >= 256 and M >= 1024 on a grid of >= 192 tiles) and under ln_stats, any
 *   float pointer on the 128x128 tile.  Only C[r][0 .. N) of the M mapped rows is written.  */
typedef struct {
  const uint16_t* A1; int32_t lda1; int32_t K1;
  const uint16_t* A2; int32_t lda2;
  const uint16_t* W;  int32_t ldw;
  const float* bias;
  const uint16_t* residual;
  uint16_t* C; int32_t ldc;
  int32_t M, N, K;
  /* act: the activation code in the low byte (0 none, 1 exact-erf GELU).  The bits above it are DIAGNOSTIC AND TEST SWITCHES, not
   * product options: a product caller passes 0 or AM_GEMM_ACT_GELU.  Every choice they make gives the same result (the tests hold
   * the tilings and the two GELU forms bit-identical); the ablations skip work and give a wrong one, for timing only. */
  int32_t act;
#define AM_GEMM_ACT_MASK      0xff     /* the activation code */
#define AM_GEMM_ACT_GELU      1
#define AM_GEMM_FORCE_128     0x100    /* the 128x128 register-staged kernel at any size (wins over FORCE_256) */
#define AM_GEMM_LOCKSTEP      0x200    /* the lockstep main loop of the 256x256 tile instead of the ping-pong loop (A/B runs) */
#define AM_GEMM_FORCE_256     0x400    /* the 256x256 tile at any grid size */
#define AM_GEMM_ABLATE_STORE  0x800    /* timing: no C store (am_gemm_headpost_bf16: no Q / K rows) */
#define AM_GEMM_ABLATE_READ   0x1000   /* timing: no residual read (am_gemm_headpost_bf16: no V^T read-back) */
#define AM_GEMM_ABLATE_MASK   0x1800
#define AM_GEMM_SKEW_SHIFT    13       /* bits 13-15: per-XCD start skew of the 256x256 grid in 1.5 us units; 0 = the library's */
#define AM_GEMM_SKEW_MASK     0xe000   /* choice, 7 = none */
#define AM_GEMM_NO_GELU_TABLE 0x10000  /* the arithmetic GELU epilogue in the 256x256 tile too (default: the bit-identical table) */
  int32_t a_G, a_gs, a_off;
  int32_t c_G, c_gs, c_off;
  /* LayerNorm folded into the linear that consumes it (block.py:138,146,152: norm -> to_q|k|v / to_q / ff.net.0): with
   * ln_stats != NULL, A holds the UN-normalised rows x, W holds bf16(W (.) gamma), `bias` holds d = W beta + b,
   * ln_colsum[n] = sum_k W'[n][k], ln_stats[r] = (mean_r, rstd_r) (am_row_stats_bf16 / am_row_stats_finalize), and
   *   C = act(rstd_r (x W'^T - mean_r colsum) + d) + residual
   * - the normalised activation is never written.  Identity A row map, no A2.  am_ln_fold_weight prepares W', colsum, d. */
  const float* ln_stats;
  const float* ln_colsum;
  /* LayerNorm statistics of the OUTPUT rows for the next consumer (written, not read): ln_part [M][ceil(N / 256)] pairs
   * (mean, M2) of each row's 256-column slice of the bf16-rounded C (after act + residual); am_row_stats_finalize merges them. */
  float* ln_part;
} am_gemm_args;
int am_gemm_bf16(const am_gemm_args* args, void* stream);

/* (mean, rstd) of every row of x [rows][C] bf16, fp32 two-pass statistics (the ones am_layernorm_bf16 uses). */
int am_row_stats_bf16(const uint16_t* x, float* stats, int64_t rows, int C, float eps, void* stream);
/* Merge the per-slice (mean, M2) pairs a producer GEMM wrote (am_gemm_args.ln_part, `nparts` = ceil(C / 256) slices of 256
 * columns, the last one shorter when C % 256 != 0) into (mean, rstd) per row - Chan's pairwise update, no E[x^2] - mean^2 cancellation. */
int am_row_stats_finalize(const float* part, int nparts, int C, float* stats, int64_t rows, float eps, void* stream);
/* am_layernorm_bf16 that also writes (mean, rstd) of its bf16-rounded OUTPUT rows to stats_y [rows][2] (block.py:133 -> :138:
 * norm_skip's output is the input of the next, folded, LayerNorm). */
int am_layernorm_stats_bf16(const uint16_t* x, uint16_t* y, const float* w, const float* b,
                            int64_t rows, int C, float eps, float* stats_y, void* stream);
/* One-time weight preparation of a folded linear: Wf = bf16(W (.) gamma) [N][K], colsum[n] = sum_k Wf[n][k],
 * d[n] = sum_k W[n][k] beta[k] + bias[n] (bias may be NULL).  W is the bf16 weight the un-folded linear uses. */
int am_ln_fold_weight(const uint16_t* W, const float* gamma, const float* beta, const float* bias, uint16_t* Wf, float* colsum,
                      float* d, int N, int K, void* stream);

/* FP32LayerNorm / nn.LayerNorm (block.py:64,83,98,107; temporal_denoiser.py:107):
 * y = (x-mean)/sqrt(var+eps)*w+b, fp32 statistics, bf16 in/out. C % 8 == 0, C <= 4096. */
int am_layernorm_bf16(const uint16_t* x, uint16_t* y, const float* w, const float* b,
                      int64_t rows, int C, float eps, void* stream);

/* fp32 residual stream (Stage II, temporal_autoencoder.py:258: the reference's torch.cat promotes its residual stream to fp32, every
 * `h + branch` under autocast adds a 16-bit linear output into it, FP32LayerNorm reads it in fp32 and the next autocast linear rounds its
 * input to 16 bits; the DINOv2 encoder, image_encoder.py:38-55 / pipeline.py:665-667, runs in fp32).  One pass:
 *   h32 [rows][C] += y16 [rows][C]   (the branch's 16-bit output; NULL: nothing to add),
 *   z16 [rows][C]  = LayerNorm(h32) * w + b, rounded to 16 bits   (NULL: accumulate only).   C % 8 == 0, C <= 4096. */
int am_add_layernorm_f32(float* h32, const uint16_t* y16, uint16_t* z16, const float* w, const float* b, int64_t rows, int C, float eps,
                         void* stream);

/* Head split + qk RMSNorm + RoPE + attention operand layout
 * (attention_processor.py:106-130).
 *   X [rows][ldx] bf16; head h, part p at columns (h*nparts + p)*128.
 *   rows are grouped in sequences of `seq_len` rows; each sequence is
 *   `seq_len / rows_per_frame` frames; the RoPE row of a token is its global
 *   frame index  (row / rows_per_frame).
 *   part kinds: 0 = Q-like (RMSNorm w0, optional RoPE) -> out0 [nseq][H][s0_pad][128]
 *               1 = K-like (RMSNorm w1, optional RoPE) -> out1 [nseq][H][s1_pad][128]
 *               2 = V      (copy)                      -> out2 [nseq][H][128][s1_pad], keys
 *                   permuted inside each group of 16 (bit2<->bit3) for the PV MFMA.  */
typedef struct {
  const uint16_t* X; int32_t ldx;
  int64_t rows; int32_t seq_len; int32_t rows_per_frame;
  int32_t heads; int32_t nparts; int32_t kinds[3];
  const float* w_q; const float* w_k; float eps;
  const float* rope_cos; const float* rope_sin;   /* [frames][64] or NULL */
  uint16_t* out_q; int32_t sq_pad;
  uint16_t* out_k; uint16_t* out_vt; int32_t sk_pad;
} am_headpost_args;
int am_head_post(const am_headpost_args* args, void* stream);

/* The bias-free q | k | v projection (or the cross-attention to_q) AND am_head_post in one launch (north_star's "fused RMSNorm + RoPE +
 * QKV"; attention_processor.py:92-130): the head split, qk-RMSNorm, RoPE and the operand layouts run in the GEMM's epilogue on the
 * bf16-rounded linear output - bit-identical to am_gemm_bf16 followed by am_head_post, without the (rows x N) activation round trip.
 * `gemm` as for am_gemm_bf16 with C = headpost->X, ldc = headpost->ldx, M = headpost->rows, N = heads * nparts * 128 (X is still needed:
 * the remainder rows of the tile grid go through it).  Shapes that do not qualify run the two calls instead - same results. */
int am_gemm_headpost_bf16(const am_gemm_args* gemm, const am_headpost_args* headpost, void* stream);

/* F.scaled_dot_product_attention, non-causal, head_dim 128
 * (attention_processor.py:133-139).  Online-softmax flash kernel on bf16 MFMA.
 *   Q  [nseq][H][sq_pad][128]; K [chunks][nseq][H][sk_pad][128];
 *   Vt [chunks][nseq][H][128][sk_pad] (permuted as am_head_post writes it);
 *   O  [nseq*sq][ldo] at column h*128 (heads concatenated, token-major).
 *   Each chunk holds `sk` valid keys.  sq_pad % 256 == 0, sk_pad % 64 == 0. */
typedef struct {
  const uint16_t* Q; const uint16_t* K; const uint16_t* Vt; uint16_t* O;
  int32_t nseq, heads, sq, sq_pad, sk, sk_pad, nchunks;
  int64_t chunk_stride;        /* elements between consecutive chunks of K (and of Vt) */
  int32_t ldo; float scale; int32_t defer_log2;
  /* Two-pass attention over a key stream that arrives in pieces (multi-GPU: the local K/V shard is there before
   * the all-gather of the others completes).  All zero = one pass over chunks 0 .. nchunks-1.
   *   chunk_total > 0: the `nchunks` chunks walked are (chunk_first + i) % chunk_total, i = 0 .. nchunks-1;
   *   rows: 0 = all query blocks, 1 = the full 256-row blocks a long key stream runs on the 4x64 kernel ("main"),
   *         2 = whatever `rows = 1` leaves out (the short last block);
   *   state_mode (rows = 1 only): 1 = stop after these chunks and save the un-normalised (O, m, l) of every row
   *         to `state` ([nseq*heads][sq_pad][132] floats), writing no output; 2 = start from `state`, finish, write O. */
  int32_t chunk_first, chunk_total, rows, state_mode;
  float* state;
} am_attn_args;
/* Floats per query row of `state`: O[128], m, l, pad (16-byte aligned rows). */
#define AM_ATTN_STATE_LD 132
/* am_attn_args.defer_log2 as am_attention_bf16 reads it.  A product caller passes one of the two re-base thresholds:
 *   AM_ATTN_REBASE_ALWAYS    exact online softmax, re-based whenever a row max grows;
 *   AM_ATTN_REBASE_DEFERRED  the product: deferred re-base (threshold 2^8) on the 8-wave kernel, the lazy re-base of the 4x64 kernel
 *                            (+ its exact fallback launch) on long key streams.
 * The product dispatch picks the kernel from the shape (short key streams: the 8-wave code in its 4-wave geometry or the
 * resident-key-stream kernel; long ones: the 4x64 kernel).  Every other code is a DIAGNOSTIC AND TEST SWITCH that forces one kernel
 * for A/B runs and parity tests: a base below plus one of the two thresholds. */
#define AM_ATTN_REBASE_ALWAYS   0
#define AM_ATTN_REBASE_DEFERRED 8
#define AM_ATTN_4WAVE           50     /* + threshold: the 8-wave kernel's code as two 4-wave workgroups per CU (geometry A/B) */
#define AM_ATTN_4X64            60     /* + threshold: 4 waves x 64 rows, one wave per SIMD */
#define AM_ATTN_BALANCED        70     /* + threshold: the balanced two-phase schedule of the 8-wave kernel */
#define AM_ATTN_8WAVE           90     /* + threshold: the 8-wave kernel at any key-stream length */
#define AM_ATTN_4X64_DEFERRED   28     /* the 4x64 kernel with the exact deferred re-base on its own (no lazy pass) */
/* builds with -DAM_ATTN_ABLATIONS only (tools/kernel_bench.py): the experimental schedules of the A/B build from this code on, and
 * from AM_ATTN_ABLATE_4X64 on the 4x64 kernel's timing ablations (+ ABL; numerically meaningless) */
#define AM_ATTN_VARIANTS        100
#define AM_ATTN_ABLATE_4X64     3000
/* am_attn_args.defer_log2 as am_attention_fp8 reads it: 0 = the product dispatch (the free-running kernel for key streams of at least
 * 8 tiles, the 8-wave kernel below); otherwise one of these bases.  The "+ ABL" forms are timing ablations of the one-pass form. */
#define AM_ATTN_FP8_ABLATE         5000   /* + ABL: the 8-wave kernel and its timing ablations */
#define AM_ATTN_FP8_4X64           5100   /* + ABL: the 4 x 64 form (same-box A/B) */
#define AM_ATTN_FP8_8WAVE          5200   /* the 8-wave kernel at any key-stream length (same-box A/B, tests) */
#define AM_ATTN_FP8_PRODUCT_ABLATE 5300   /* + ABL: timing ablations of the product (free-running) kernel */
#define AM_ATTN_FP8_FAST           5400   /* the product kernel with the exponent-field form of the probabilities (am_config.attn_fp8 = 2) */
int am_attention_bf16(const am_attn_args* args, void* stream);
/* Diagnostic: the long-key-stream kernel keeps no running row max in its loop (it re-bases lazily from the row sums);
 * a workgroup that meets a single-tile jump of more than 2^60 is recomputed by an exact kernel launched behind it.
 * Returns how many workgroups that fallback has recomputed on the current device so far (synchronises the device). */
int am_attention_fallback_count(uint64_t* count);

/* fp8 (OCP e4m3) variant of the same attention (BASELINE.json configs[4]: "fp8 MFMA"): QK^T and P.V on the MX-scaled
 * K = 64 MFMA (block scales 2^0), fp32 online softmax, bf16 output.  Two calls: quantise the bf16 operand layouts that
 * am_head_post writes (Q pre-multiplied by scale * log2 e; V^T re-ordered to the key order of the fp8 P.V operand), then
 * attend.  q8 / k8 / vt8 have the element counts and strides of Q / K / Vt (one byte per element; chunk_stride counts
 * bytes).  The forms of am_attention_bf16 (round 3): chunk_first / chunk_total ring walks (the quantiser converts exactly the
 * chunks an attention call with the same arguments walks; rows = 2 skips Q), rows = 1 / 2, state_mode 1 / 2 with the same
 * [seq*heads][sq_pad][132] state layout, and the short last query block split over the key range.  Stated tolerance vs fp32
 * SDPA: tests/test_attention_fp8.py.
 * The quantiser is round-to-nearest-even e4m3 of the fp32 value (Q: times the fp32 product scale * log2 e), bit for bit torch's
 * x.clamp(-448, 448).to(float8_e4m3fn): +-inf and everything beyond +-448 saturate to +-448, a NaN stays a NaN (0x7f under either sign bit), -0 and
 * what rounds to it keep their sign, subnormals are multiples of 2^-9 with ties to even (2^-10 -> 0, 3 x 2^-10 -> 2^-8).
 * Range of the probabilities, per form (am_attention_fp8.hip's header has the reasons; tests/test_fp8_range_gpu.py holds each
 * form to it against the fp64 emulator of tests/_fp8_range.py):
 *   - numerator: a key seen d octaves under the running maximum counts iff d < 15 (the 8-wave, 4 x 64 and product kernels: e4m3 of
 *     2^(5 - d), the 2^-10 tie goes to 0) or d < 12 (AM_ATTN_FP8_FAST: linear subnormals from d = 11 on).  A key seen BEFORE the
 *     maximum rises is rescaled in fp32 and never lost, so the keys lost depend on the order of the walk: one pass, a rank's
 *     two-pass ring order, the independent key ranges of the split last block.
 *   - row sum: the 8-wave kernel (also every short last block and every stream under 8 tiles) and the 4 x 64 kernel add the
 *     unrounded fp32 probabilities - the output shrinks by the lost share of the softmax mass; the product kernel and
 *     AM_ATTN_FP8_FAST add the rounded e4m3 ones - the softmax renormalises over the surviving keys (V = 1 gives 1).
 *   - non-finite operands: a NaN in V poisons its channel in every row of the head, a NaN in a query row that output row, in every
 *     form; a NaN in a key row makes every row of the head NaN, except under AM_ATTN_FP8_FAST, which drops that key silently (its
 *     byte convert writes 0 for a NaN score) and stays finite. */
int am_attention_quantize_fp8(const am_attn_args* args, uint8_t* q8, uint8_t* k8, uint8_t* vt8, void* stream);
int am_attention_fp8(const am_attn_args* args, const uint8_t* q8, const uint8_t* k8, const uint8_t* vt8, void* stream);

/* Copy-engine exchange of the K / V^T shards between ranks (multi-GPU, one process per GPU; the alternative to the RCCL
 * all-gather of seam S2's phase API, sharding.py PeerExchange): IPC-shareable device buffers, SDMA copies between them, and
 * sequence flags written / awaited in stream order by one-lane kernels.
 *   am_peer_alloc / free      hipMalloc'd (zeroed) buffer whose IPC handle can be exported
 *   am_peer_export / open / close   64-byte HIP IPC handle <-> mapped pointer in another process of the node
 *   am_peer_copy              asynchronous device-to-device copy on `stream` (copy engines, no CU)
 *   am_peer_signal            *flag = value (system-scope release) after everything earlier on `stream`
 *   am_peer_wait              holds `stream` until (int32)(*flag - value) >= 0; gives up after ~20 s and sets *fault_word */
int am_peer_alloc(size_t bytes, void** dev_ptr);
/* The flag block of an exchange (polled by a kernel of the owning device while a PEER device writes it): device-local FINE-GRAINED
 * memory (hipExtMallocWithFlags(hipDeviceMallocFinegrained)), zeroed, IPC-exportable like am_peer_alloc's; *fine_grained = 1, or 0
 * when the runtime refused and an ordinary allocation was returned instead.  Free with am_peer_free. */
int am_peer_alloc_flags(size_t bytes, void** dev_ptr, int* fine_grained);
int am_peer_free(void* dev_ptr);
int am_peer_export(void* dev_ptr, uint8_t* handle64);
int am_peer_open(const uint8_t* handle64, void** dev_ptr);
int am_peer_close(void* dev_ptr);
int am_peer_copy(void* dst_dev, const void* src_dev, size_t bytes, void* stream);
int am_peer_signal(uint32_t* flag_dev, uint32_t value, void* stream);
int am_peer_wait(const uint32_t* flag_dev, uint32_t value, uint32_t* fault_word_dev, void* stream);

/* Diagnostic: while a trace is open, every kernel of the phase API (am_forward_begin .. am_forward_end) is followed by a
 * position-weighted integer checksum of its output, appended in stream order to `log_dev` (capacity uint64 words, zeroed by the
 * caller).  am_debug_trace_end closes the trace and returns the entries' tags (stage * 100 + layer; am_debug_trace_stage_name).
 * Process-wide, single-threaded like the rest of the API; used by tools/peer_selftest.py --ktrace to find which kernel's output
 * moves between two forwards on bit-identical inputs. */
int am_debug_trace_begin(uint64_t* log_dev, int capacity);
int am_debug_trace_end(int32_t* tags_host, int capacity, int* n_entries);
const char* am_debug_trace_stage_name(int stage);

/* small fused elementwise ops */
int am_f32_to_bf16(const float* x, uint16_t* y, size_t n, void* stream);
int am_bf16_to_f32(const uint16_t* x, float* y, size_t n, void* stream);
/* diffusers Timesteps(flip_sin_to_cos=False, shift=0): [sin(t f) | cos(t f)] -> bf16 (rows, C) */
int am_timestep_sinusoid(const float* t_dev, uint16_t* out, int rows, int C, void* stream);

/* Stage II (ActionMeshAutoencoder, temporal_autoencoder.py) featurisation around the kernels above:
 *   am_point_embed: FrequencyPositionalEmbedding (embeddings.py:14-52) of query (rows, ld_in) fp32 = [xyz | extra] ->
 *                   bf16 (rows, ld_out) = [x | sin(x f) | cos(x f) | extra | 0 pad], f_j = 2^j (* pi if include_pi)
 *   am_displacement: out (rows, out_dim) fp32 = 2 sigmoid(-logits) - 1   (temporal_autoencoder.py:156-157, 267) */
int am_point_embed(const float* q_dev, int ld_in, int64_t rows, int in_channels, int extra_channels, int num_freqs,
                   int include_pi, uint16_t* out, int ld_out, void* stream);
int am_displacement(const uint16_t* logits, int ld, int64_t rows, int out_dim, float* out, void* stream);

/* Context encoder (image_encoder.py:38-55 -> transformers Dinov2PatchEmbeddings): im2col of the kernel = stride patch
 * convolution, pixels (frames, channels, height, width) fp32 -> bf16 (frames * (height/patch) * (width/patch), ld_out),
 * columns in flattened-Conv2d-weight order (c, ky, kx), zero padded to ld_out; the projection itself is am_gemm_bf16. */
int am_patchify(const float* pixels, int frames, int channels, int height, int width, int patch, uint16_t* out,
                int ld_out, void* stream);

/* ---- exact-fp32 matrix path (csrc/am_f32.hip; v_mfma_f32_32x32x2_f32: fp32 operands and accumulation) ------------------------
 * What the reference computes with autocast off: Stage II's query embedding, proj_query, the cross-attention FlowMatchingBlock,
 * norm_out and proj_out (temporal_autoencoder.py:152-161, 240-243, 266-267), and the DINOv2 encoder (pipeline.py:665-667,
 * image_encoder.py:38-55).  fp32 pointers, row-major; deterministic (no split-K, no atomics); the same bits from both library builds.
 *
 * nn.Linear in fp32 (block.py linears, proj_query / proj_out, Dinov2 query / key / value / dense / fc1 / fc2):
 *   C[M][ldc] = act(A[M][lda] W^T + bias[N]) + R[M][ldr], W [N][ldw] (nn.Linear layout), bias / R may be NULL, R may alias C.
 *   act 0 = none, 1 = exact erf-GELU (F.gelu).  Any M, N; K % 4 == 0; A, W 16-byte aligned, lda, ldw multiples of 4. */
int am_gemm_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias, const float* R, int64_t ldr,
                float* C, int64_t ldc, int M, int N, int K, int act, void* stream);
/* softmax(Q K^T * scale) V per (sequence, head), non-causal, fp32 (F.scaled_dot_product_attention in attention_processor.py:145,
 * Dinov2SelfAttention).  Operands are read in place from projection outputs: element d of head h of row i of sequence n of X is
 *   X[(n * s + i) * ldx + x_off + h * x_hs + d]     (s = sq for Q, sk for K / V)
 * so the reference's per-head split of the CONCATENATED cross-attention projection (attention_processor.py:105-115: K of head h at
 * column h * 2 hd of [to_k | to_v], V at h * 2 hd + hd) and transformers' h * hd split are both just strides.
 * O [nseq * sq][ldo], heads concatenated (h * head_dim + d).  head_dim 64 or 128; sq, sk >= 1; pointers, ld*, *_off and *_hs aligned
 * to 16 bytes.  Exact online softmax (running row max), libm expf. */
typedef struct {
  const float* Q; int64_t ldq; int32_t q_off, q_hs;
  const float* K; int64_t ldk; int32_t k_off, k_hs;
  const float* V; int64_t ldv; int32_t v_off, v_hs;
  float* O; int64_t ldo;
  int32_t nseq, heads, sq, sk, head_dim;
  float scale;
} am_attn_f32_args;
int am_attention_f32(const am_attn_f32_args* args, void* stream);
/* nn.LayerNorm / FP32LayerNorm in fp32 (block.py:64,83,98,107 with eps 1e-5; Dinov2Layer norm1 / norm2 / layernorm with eps 1e-6):
 * y = (x - mean) / sqrt(var + eps) * w + b, two-pass statistics.  C % 4 == 0, C <= 4096; y may not alias x. */
int am_layernorm_f32(const float* x, float* y, const float* w, const float* b, int64_t rows, int C, float eps, void* stream);
/* fp32-output forms of am_point_embed / am_patchify (same element maps, no rounding) and am_displacement on fp32 logits
 * (2 sigmoid(-logits) - 1, temporal_autoencoder.py:156-157, 267). */
int am_point_embed_f32(const float* q_dev, int ld_in, int64_t rows, int in_channels, int extra_channels, int num_freqs,
                       int include_pi, float* out, int ld_out, void* stream);
int am_patchify_f32(const float* pixels, int frames, int channels, int height, int width, int patch, float* out, int ld_out,
                    void* stream);
int am_displacement_f32(const float* logits, int ld, int64_t rows, int out_dim, float* out, void* stream);

/* ---- exact-fp32 Stage I (csrc/am_stage1_f32.hip): what HipDenoiser(dtype="float32") needs beside the matrix path above ----------
 * fp32 and nothing narrower, every operation rounded once in the order written here (built without contraction into fused
 * multiply-adds); deterministic; the same bits from both library builds.
 *
 * qk-RMSNorm (diffusers RMSNorm(dim_head, eps), attention_processor.py:121-124) and RoPE (rotary_embedding.py:72-124,
 * attention_processor.py:127-130) IN PLACE on the 128-wide head chunks of a packed fp32 projection output, addressed as
 * am_attention_f32 addresses them: the chunk of head h of row r is x = X[r * ldx + off + h * head_stride .. + 128].  Per chunk:
 *   ss   = sum of x[d] * x[d]: per lane (x0 x0 + x1 x1) + (x2 x2 + x3 x3) of four consecutive d, then a binary tree over the 32 lanes
 *          (8 levels in all, the same tree every launch)
 *   r    = 1 / sqrt(ss / 128 + eps)
 *   y[d] = (x[d] * r) * w[d]                                              w [128]
 *   with tables (rope_cos, rope_sin: [frames][64] fp32, one value per interleaved pair, frame = r / rows_per_frame):
 *   c = rope_cos[frame][i], s = rope_sin[frame][i]:   out[2i] = y[2i] * c + (-y[2i + 1]) * s,   out[2i + 1] = y[2i + 1] * c + y[2i] * s
 * and out (or y, with NULL tables: frames and rows_per_frame are then ignored) is written back over x.  One launch handles ONE chunk
 * kind: the caller launches it for q and for k (cross-attention: for q, and for the context's k).  No column outside the addressed
 * chunks is read or written.  X, w 16-byte aligned; ldx, off, head_stride multiples of 4; head_stride >= 128 unless heads == 1;
 * off + (heads - 1) * head_stride + 128 <= ldx; (rows - 1) / rows_per_frame < frames. */
int am_head_post_f32(float* X, int64_t ldx, int off, int head_stride, int64_t rows, int heads, const float* w, float eps,
                     const float* rope_cos, const float* rope_sin, int frames, int rows_per_frame, void* stream);
/* RoPE alone, for the self-attention of Stage II, which rotates q and k WITHOUT a qk-norm (attention_qk_norm=None,
 * temporal_autoencoder.py:83-92; am_head_post_f32 always normalises and refuses a null gain).  IN PLACE on the 128-wide head chunks of a
 * packed fp32 projection output, addressed as above, TWO chunk kinds in one launch: x = X[r * ldx + off_a + h * head_stride .. + 128]
 * (q) and, unless off_b < 0 (one kind only), X[r * ldx + off_b + h * head_stride .. + 128] (k).  With c = rope_cos[frame][i],
 * s = rope_sin[frame][i], frame = r / rows_per_frame (tables [frames][64] fp32, both required):
 *   out[2i] = x[2i] * c + (-x[2i + 1]) * s,   out[2i + 1] = x[2i + 1] * c + x[2i] * s
 * two products and one sum per element, each rounded once to fp32 in that order: the bits of the unfused torch fp32 expression
 * x * cos + rot(x) * sin (rotary_embedding.py:72-124).  No column outside the addressed chunks - the v chunks, padding behind the last
 * chunk - is read or written.  X 16-byte aligned; ldx, off_a, off_b, head_stride multiples of 4; head_stride >= 128 unless heads == 1;
 * off_x + (heads - 1) * head_stride + 128 <= ldx for both kinds; no q chunk may overlap a k chunk; (rows - 1) / rows_per_frame < frames.
 * A refused call launches nothing. */
int am_rope_f32(float* X, int64_t ldx, int off_a, int off_b, int head_stride, int64_t rows, int heads, const float* rope_cos,
                const float* rope_sin, int frames, int rows_per_frame, void* stream);
/* The fp32 form of am_flow_step: ClassifierFreeGuidance.aggregate_cfg (guidance.py:95-118) and the Euler step with its masked write
 * (scheduler.py:238-248) as the reference computes them in fp32 - the bits of the torch fp32 expression:
 *   out = v_0;   out = out + scale_i * (v_{i+1} - v_i)   for i = 0 .. n_branches - 2   (a subtraction, a product, a sum: three roundings)
 *   step = dt * out;   latents[f] = latents[f] + step (is_additive) or latents[f] - step   for frames with unobserved[f] != 0
 * (unobserved_host NULL: every frame).  latents_dev fp32 (T_local, N, Din), v_dev fp32 (n_branches, T_local, N, Din); frames that are
 * not unobserved are neither read nor written.  n_branches 1 .. 4, T_local <= 256. */
int am_flow_step_f32(const float* v_dev, float* latents_dev, int n_branches, const float* scales_host, float dt, int is_additive,
                     const uint8_t* unobserved_host, int T_local, int N, int Din, void* stream);

/* ActionBench quality gate (actionbench/chamfer.py:13-86, actionbench/icp.py:94): exact nearest-neighbour
 * search, the arithmetic of scipy.spatial.KDTree(points).query(queries) and of pytorch3d's chamfer_distance.
 *   points  (batch, n_points, 3) fp32, batch stride points_bstride ELEMENTS (0 = one cloud shared by every batch entry);
 *   queries (batch, n_queries, 3) fp32 likewise;
 *   out_index (batch, n_queries) int32 = argmin_p |q - p|^2, ties -> lowest index;
 *   out_d2    (batch, n_queries)       = that minimum SQUARED distance, double when precise != 0 (fp64 arithmetic,
 *             ((dx*dx) + (dy*dy)) + dz*dz without contraction: bit-identical to the reference's KD-tree), else float.
 * am_nn_workspace_bytes() bytes of device scratch (may be 0) must be passed for the same (n_points, n_queries, batch, precise). */
typedef struct {
  const float* points;
  int64_t n_points;
  int64_t points_bstride;
  const float* queries;
  int64_t n_queries;
  int64_t queries_bstride;
  int32_t batch;
  int32_t precise;
  int32_t* out_index;
  void* out_d2;
} am_nn_args;
size_t am_nn_workspace_bytes(int64_t n_points, int64_t n_queries, int batch, int precise);
int am_nn_search(const am_nn_args* args, void* workspace_dev, size_t workspace_bytes, void* stream);

/* The same search through a uniform grid (csrc/am_nn_grid.hip): out_index and out_d2 are am_nn_search's BIT FOR BIT - the same
 * d2 = ((dx*dx) + (dy*dy)) + dz*dz in fp32 or fp64 without contraction, the minimum over all points, ties to the lowest index,
 * index -1 with d2 = +inf when no distance is finite - while only the points of a growing cube of cells are evaluated.  General
 * purpose and exact; what it buys depends on how close the clouds lie (profiles/nn_grid.json).
 *
 * THE GRID of one cloud of n_points (batch entries are independent), G = cells per axis, 1 .. 128.  All arithmetic is fp32, each
 * operation rounded on its own, fl() below:
 *   frame       float[8] = { lo_x, lo_y, lo_z, 0, inv_x, inv_y, inv_z, 0 }.  lo_k / hi_k: the minimum / maximum of coordinate k
 *               over the points whose three coordinates are all finite, in the total order of the IEEE bit patterns (-0 below +0);
 *               no such point: lo = 0, inv = 0.  inv_k = fl(G / fl(hi_k - lo_k)); when the extent is 0 or that quotient is not
 *               finite, inv_k = 0.
 *   cell of p   c_k = the clamped cell of step 2 of THE SEARCH below, of p_k in place of q_k (for a finite point of this cloud
 *               0 <= t, so c_k = min(G - 1, (int)floorf(t))); cell = (c_z * G + c_y) * G + c_x.  A point with a non-finite
 *               coordinate goes to the extra cell G^3 and never matches.
 *   order       int32[n_points]: the point indices sorted by (cell, index) - ties inside a cell in ascending index, so every array
 *               here is defined bit for bit.
 *   cell_start  int32[G^3 + 2]: cell_start[c] = number of points in cells below c; [G^3] starts the extra cell, [G^3 + 1] = n_points.
 *   sorted      float[n_points][4] = { x, y, z, index bits } of the points in `order` (16-byte records).
 *   slabs       float[2][3][G]: [0][k][j] = the smallest coordinate k over the finite points with c_k >= j (suffix minimum, +inf when
 *               there is none), [1][k][j] = the largest coordinate k over those with c_k <= j (prefix maximum, -inf when none).
 * am_nn_grid_bytes(n_points, batch, cells) is the size of ONE allocation that holds frame, slabs, cell_start, order and sorted of
 * `batch` grids in that order, each array padded to a multiple of 16 bytes; every pointer must be 16-byte aligned.
 *
 * BUILDING takes two calls around a sort that is the caller's (any stable sort of out_cell; the Python binding uses torch's):
 *   am_nn_grid_cells  writes grid.frame and out_cell (batch, n_points) = the cell of every point;
 *   [caller]          grid.order = the stable argsort of out_cell along the points;
 *   am_nn_grid_build  reads grid.frame and grid.order, writes grid.sorted, grid.cell_start and grid.slabs.
 * Both need am_nn_grid_workspace_bytes(n_points, batch, cells) bytes of 16-byte aligned device scratch, whose content on entry is
 * irrelevant.  No float atomics: extrema go through integer atomics on the order-preserving map of the bit patterns.
 *
 * THE SEARCH of a query q (one lane per query; `query_order`, optional, an int32 permutation of the queries (batch stride
 * query_order_bstride elements, 0 = shared) that says in which order lanes pick queries - pass the cell order of the query cloud and
 * a wave shares cells; results are always written at the query's own position):
 *   1. a query with a non-finite coordinate has no finite distance: index -1, d2 = +inf.
 *   2. its cell is the clamped one: per axis 0 when inv_k == 0 or t = fl(fl(q_k - lo_k) * inv_k) is not >= 0, G - 1 when t >= G,
 *      else (int)floorf(t).  c_k(.) is monotone (non-decreasing) in the coordinate: it composes monotone roundings.
 *   3. rings r = 0, 1, ... : all cells at Chebyshev distance r from that cell, inside the grid; every point of them is evaluated with
 *      the arithmetic above (T = float or double, operands converted first) and the best (d2, index) is kept lexicographically.
 *   4. after ring r, per axis k and side: high side g = fl_T(slabs[0][k][c_k + r + 1] - q_k), low side g = fl_T(q_k -
 *      slabs[1][k][c_k - r - 1]); a side whose slab index leaves 0 .. G - 1 is exhausted (g = +inf).
 *   5. stop when every side is exhausted, or when best < fl_T(g_min * g_min), g_min the smallest of the six; at most G rings.
 * WHY THIS IS EXACT.  A point p outside the cube of rings 0 .. r has, on some axis k, c_k(p) >= c_k(q) + r + 1 or <= c_k(q) - r - 1.
 * High side: c_k is monotone and c_k(p) > c_k(q), so p_k > q_k for every such p, hence the slab minimum m satisfies p_k >= m >= q_k;
 * rounding is monotone, so |fl(q_k - p_k)| = fl(p_k - q_k) >= fl(m - q_k) = g >= 0, then fl(dx dx) >= fl(g g), and a rounded sum of
 * non-negative terms is no smaller than either term: d2(p) >= fl(g g) >= fl(g_min g_min) > best.  The low side mirrors it.  So no
 * point outside the cube beats OR TIES the best; nothing rests on where a cell's edge falls after rounding.  Points of the extra
 * cell have no finite distance and are never the answer of am_nn_search either.
 *
 * Every cell_start value, every index of `sorted`, every `order` and `query_order` entry is compared with its bound before it is used
 * as an address or written as a result; a violation sets a bit of out_flag (device int32[1], zeroed by the call) and the element
 * concerned is written as "no neighbour" (index -1, d2 +inf; a bad `order` entry as a NaN record in the extra cell; a bad
 * `query_order` entry names no position and is skipped): a bad grid reports an error and nothing outside the outputs is written.  The status is AM_OK; the caller reads the flag. */
#define AM_NN_GRID_MAX_CELLS 128
#define AM_NN_GRID_BAD_ORDER 1         /* am_nn_grid_build: an `order` entry outside [0, n_points) */
#define AM_NN_GRID_BAD_CELL_START 2    /* am_nn_grid_search: cell_start not ascending inside [0, n_points] */
#define AM_NN_GRID_BAD_INDEX 4         /* am_nn_grid_search: an index of `sorted` outside [0, n_points) */
#define AM_NN_GRID_BAD_QUERY_ORDER 8   /* am_nn_grid_search: a `query_order` entry outside [0, n_queries) */
typedef struct {
  int64_t n_points;
  int32_t batch;      /* number of grids; a search of more batch entries than 1 may share ONE grid (batch == 1) */
  int32_t cells;      /* G */
  float* frame;
  float* slabs;
  int32_t* cell_start;
  int32_t* order;
  float* sorted;
} am_nn_grid;
typedef struct {
  const float* points;      /* (batch, n_points, 3) fp32 */
  int64_t points_bstride;   /* elements; 0 = one cloud for every grid */
  am_nn_grid grid;
  int32_t* out_cell;        /* am_nn_grid_cells only: (batch, n_points) */
  int32_t* out_flag;        /* am_nn_grid_build only */
  void* workspace;
  size_t workspace_bytes;
} am_nn_grid_build_args;
typedef struct {
  am_nn_grid grid;
  const float* queries;     /* (batch, n_queries, 3) fp32 */
  int64_t n_queries;
  int64_t queries_bstride;  /* elements; 0 = shared */
  int32_t batch;
  int32_t precise;
  const int32_t* query_order;
  int64_t query_order_bstride;
  int32_t* out_index;       /* (batch, n_queries) */
  void* out_d2;             /* (batch, n_queries) double when precise != 0, else float */
  int32_t* out_flag;
} am_nn_grid_search_args;
size_t am_nn_grid_bytes(int64_t n_points, int batch, int cells);
size_t am_nn_grid_workspace_bytes(int64_t n_points, int batch, int cells);
int am_nn_grid_cells(const am_nn_grid_build_args* args, void* stream);
int am_nn_grid_build(const am_nn_grid_build_args* args, void* stream);
int am_nn_grid_search(const am_nn_grid_search_args* args, void* stream);

/* One iteration of the ActionBench ICP on the device (csrc/am_icp.hip; actionbench/icp.py:86-106): the two nearest-neighbour matchings
 * of the Chamfer loss, its gradient with respect to the 12 parameters of every candidate, one Adam step and the best-so-far record,
 * without an index tensor, a gather, a scatter or a host read.  B = batch candidates share pred (P = n_pred points p_i) and gt
 * (Q = n_gt points y_j).  fl32 / fl64: one operation rounded on its own, no contraction anywhere; dot(u, v) = (u0 v0 + u1 v1) + u2 v2
 * and cross(u, v) = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0), two products and one difference each.
 *
 * params (B, 12) fp32 = [T (3), d6 (6), s (3)] per candidate.  Everything below is per candidate b.
 *  1. THE ROTATION, fp64 on the widened fp32 values: a1 = d6[0:3], a2 = d6[3:6];
 *       n1 = max(sqrt(dot(a1, a1)), 1e-12), b1 = a1 / n1;  d = dot(b1, a2), u = a2 - d b1;
 *       n2 = max(sqrt(dot(u, u)), 1e-12), b2 = u / n2;  b3 = cross(b1, b2);  G = rows (b1, b2, b3);
 *       R64[a][j] = (Ri[a][0] G[0][j] + Ri[a][1] G[1][j]) + Ri[a][2] G[2][j] with Ri = rot_init[b] (row-major 3 x 3);
 *       R = fl32(R64) = out_rot[b]: the ONE matrix that the points, the gradient of s and the best-so-far record use.
 *  2. THE POINTS, fp32:  x_i[j] = ((fl(s0 p_i0) R[0][j] + fl(s1 p_i1) R[1][j]) + fl(s2 p_i2) R[2][j]) + T[j], formed by one device
 *     function wherever a transformed point is needed, so both directions see the same bits.
 *  3. THE MATCHING, am_nn_search's fp32 arithmetic and tie rule: d2 = (dx dx + dy dy) + dz dz, the candidates visited in ascending
 *     index and accepted on d2 < best only (best starts at +inf: the lowest index wins a tie, a NaN or infinite d2 never wins).
 *       direction 0: for every i, n(i) = argmin_j d2(x_i, y_j);   direction 1: for every j, m(j) = argmin_i d2(y_j, x_i).
 *     A query without a winner (index -1) contributes NO term, sets AM_ICP_NO_NEIGHBOUR in out_flag, and is never used as an index.
 *  4. THE 13 TERMS of a matched pair (x, y, p: the untransformed point of x), fp32 then widened:  r = x - y;
 *       [0] (r0 r0 + r1 r1) + r2 r2;   [1 + j] r_j;   [4 + 3 a + j] fl(p_a r_j).
 *     sums (B, 2, 13) fp64 = their sums per direction, in a FIXED order: inside a wave of 64 consecutive queries
 *     v[l] += v[l + off] for off = 32, 16, 8, 4, 2, 1; the 4 waves of a workgroup (256 consecutive queries) left to right; the workgroups
 *     in ascending index.  No floating-point atomics: two runs give the same bits.
 *  5. THE GRADIENT, fp64.  w0 = 1 / P, w1 = 1 / Q, c2 = 2 / B (the reference calls loss.mean().backward()).
 *       A[k] = w0 sums[0][k] + w1 sums[1][k];   out_loss = fl32(A[0]);   gT[j] = c2 A[1 + j];   M[a][j] = c2 A[4 + 3 a + j];
 *       gR[a][j] = s_a M[a][j];   gs[a] = (M[a][0] R[a][0] + M[a][1] R[a][1]) + M[a][2] R[a][2]   (R widened);
 *       gG[i][j] = (Ri[0][i] gR[0][j] + Ri[1][i] gR[1][j]) + Ri[2][i] gR[2][j];   g1, g2, g3 = the rows of gG;
 *       g1 = g1 + cross(b2, g3);   g2 = g2 + cross(g3, b1);
 *       t2 = dot(g2, b2), gu = (g2 - t2 b2) / n2;   t1 = dot(gu, b1), ga2 = gu - t1 b1;
 *       g1 = g1 - (d gu + t1 a2);   t0 = dot(g1, b1), ga1 = (g1 - t0 b1) / n1;
 *     out_grad (B, 12) fp64 = [gT, ga1, ga2, gs].
 *  6. ADAM (torch.optim.Adam's defaults), fp64 on the widened fp32 state, per parameter with its gradient g:
 *       m' = beta1 m + (1 - beta1) g;   v' = beta2 v + (1 - beta2) (g g);
 *       param' = param - (lr / bias_correction1) (m' / (sqrt(v') / sqrt(bias_correction2) + eps));
 *     params, adam_m and adam_v are rounded to fp32 once, at the store.  The caller passes bias_correction{1,2} = 1 - beta{1,2}^t of
 *     its step count t, computed in double as torch does.
 *  7. BEST SO FAR (icp.py:99-106).  best (16) fp32 = [R (9), T (3), s (3), loss]; the caller starts the loss at +inf.  With c the
 *     candidate of the smallest out_loss (accepted on < only, in ascending index: the lowest index wins a tie, a NaN never wins): if
 *     out_loss[c] < best[15], best = [out_rot[c] - the R that produced the loss -, T and s of c AFTER step 6, out_loss[c]].
 * update == 0 computes the outputs and leaves params, adam_m, adam_v and best untouched.  out_flag (device int32[1]) is only ever
 * ORed into: the caller zeroes it once and reads it after any number of steps.  The workspace holds the per-workgroup partial sums
 * and must be am_icp_workspace_bytes (0 for sizes the call would refuse) bytes, 8-byte aligned; its content on entry is irrelevant.
 * Launch plan: one pairs launch of (ceil(P / 256) + ceil(Q / 256)) x B workgroups (queries one per lane, points staged through LDS in
 * tiles of 512, transformed while staged in direction 1), then one workgroup that sums, differentiates, steps and records. */
#define AM_ICP_NO_NEIGHBOUR 1          /* out_flag: a query had no finite distance to any point (NaN / inf coordinates) */
typedef struct {
  const float* pred;        /* (n_pred, 3) */
  const float* gt;          /* (n_gt, 3) */
  const float* rot_init;    /* (batch, 9) */
  int64_t n_pred;
  int64_t n_gt;
  int32_t batch;
  int32_t update;
  float* params;            /* (batch, 12) state */
  float* adam_m;            /* (batch, 12) state */
  float* adam_v;            /* (batch, 12) state */
  float* best;              /* (16) state */
  double lr, beta1, beta2, eps, bias_correction1, bias_correction2;
  float* out_loss;          /* (batch) */
  float* out_rot;           /* (batch, 9) */
  double* out_sums;         /* (batch, 2, 13) or null */
  double* out_grad;         /* (batch, 12) or null */
  int32_t* out_flag;
} am_icp_args;
size_t am_icp_workspace_bytes(int64_t n_pred, int64_t n_gt, int batch);
int am_icp_step(const am_icp_args* args, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Preview rendering (INTEGRATION seam S6; reference actionmesh/render/{renderer,visualizer}.py, PyTorch3D's
 * MeshRasterizer + soft_normal_shading): normal maps of ONE animated mesh - n_frames vertex sets on one topology - seen by
 * n_cameras PerspectiveCameras, every (frame, camera) image of the call in a fixed number of launches.
 *   vertex normals: sum of the un-normalised cross(v2 - v1, v0 - v1) of every face on the vertex, in face-index order,
 *                   normalised with eps 1e-6 (Meshes.verts_normals_packed; no float atomics: bit-identical run to run);
 *   projection:     view = X @ R + T (row vectors), x_ndc = fx * view.x / view.z + px, y likewise, depth = view.z;
 *   raster:         at 2S x 2S, pixel centre x = 1 - (2 col + 1) / W, y = 1 - (2 row + 1) / H; covered when the three
 *                   perspective-corrected, unclipped barycentrics are all > 0; the nearest face wins, ties -> lowest index.
 *                   "> 0" is strict: a centre on an edge or on a vertex of a face is not covered by it, so a centre on the edge
 *                   two faces share belongs to neither.  The barycentrics are p_i = t_i / max(t_0 + t_1 + t_2, 1e-8),
 *                   t_i = w_i z_j z_k, w_i = edge function / (area + 1e-8); the depth is interpolated with p_i / sum(p) and a
 *                   centre whose depth comes out negative is not covered.  In exact arithmetic that depth is z_0 z_1 z_2 / sum(w_i
 *                   z_j z_k) with a positive sum, so a face with exactly one vertex behind the camera is covered nowhere.
 *                   A face is skipped (1) altogether when all three depths are negative, (2) altogether when the signed area
 *                   (twice it: the edge function of one projected vertex against the other two) is within 1e-8 of zero, and (3) at every
 *                   sub-pixel centre outside the closed box [min x, max x] x [min y, max y] of its three projected vertices -
 *                   which changes nothing for a face in front of the camera (a covered centre lies inside the triangle) and
 *                   confines a face with a vertex behind the camera, whose barycentrics are all > 0 in the cone beyond that
 *                   vertex's projection, to the part of the cone inside the box (often none of it);
 *   resolve to S x S: mask = covered sub-pixels / 4; normal of sub-pixel (2i, 2j) through n @ R + T / 2, normalised,
 *                   (n + 1) / 2, clamped; rgba8 = trunc(255 * (normal * mask + 1 - mask)), alpha = trunc(255 * mask).
 *                   An uncovered sub-pixel (2i, 2j) has n = 0.  n @ R + T / 2 can cancel: with T = (0, 0, 2) a view normal of exactly
 *                   -z (a face parallel to the image that looks at the camera) maps to 0 up to rounding and has no stable
 *                   colour - the reference's shading, not a defect here; the preview's cameras have |T| = 3.
 * offsets / corners are the vertex -> corner CSR of `faces` as am_vertex_normals defines it below (int32[n_verts + 1] and
 * int32[3 n_faces], ascending corner id): corner / 3 along a vertex's corners is its faces in face-index order, one entry per
 * occurrence, which is the order of the sum above.  Faces and CSR are validated on the device as there: every index is compared
 * with its bound before it is used as an address, a face that names a vertex outside [0, n_verts) is skipped by the normals and
 * by the raster, a bad corner adds nothing, and out_flag (device int32[1], cleared in stream order by the call) then holds
 * AM_MESH_BAD_FACE / AM_MESH_BAD_CSR; the caller, who reads the flag together with the images, treats the call as failed.
 * The optional outputs (NULL = not written) are the float forms and the 2S x 2S fragments.
 * am_render_workspace_bytes() bytes of device scratch must be passed for the same sizes. */
#define AM_RENDER_MAX_CAMERAS 16
typedef struct {
  float R[9];        /* row-major 3x3: view = X @ R + T */
  float T[3];
  float fx, fy, px, py;
} am_render_camera;
typedef struct {
  const float* verts;           /* (n_frames, n_verts, 3) fp32 */
  const int32_t* faces;         /* (n_faces, 3) int32 */
  const int32_t* offsets;       /* (n_verts + 1) int32: the vertex -> corner CSR of `faces` */
  const int32_t* corners;       /* (3 n_faces) int32 */
  int32_t n_frames;
  int32_t n_verts;
  int32_t n_faces;
  int32_t n_cameras;            /* 1 .. AM_RENDER_MAX_CAMERAS */
  am_render_camera cameras[AM_RENDER_MAX_CAMERAS];
  int32_t image_size;           /* S */
  uint8_t* out_rgba;            /* (n_frames, n_cameras, S, S, 4) */
  float* out_mask;              /* optional (n_frames, n_cameras, S, S) */
  float* out_normal;            /* optional (n_frames, n_cameras, S, S, 3): (n + 1) / 2 before the mask blend */
  int32_t* out_face;            /* optional (n_frames, n_cameras, 2S, 2S): face index, -1 = empty */
  float* out_bary;              /* optional (n_frames, n_cameras, 2S, 2S, 3): clipped barycentrics, -1 = empty */
  int32_t* out_flag;            /* int32[1]: 0, or AM_MESH_BAD_FACE | AM_MESH_BAD_CSR */
} am_render_args;
size_t am_render_workspace_bytes(int n_frames, int n_verts, int n_faces, int n_cameras, int image_size);
int am_render_normals(const am_render_args* args, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Farthest-point sampling (INTEGRATION seam S7; reference actionmesh/model/utils/pointcloud_sampling.py, which on CUDA calls
 * pytorch3d.ops.sample_farthest_points - the reduction of 8192 surface points to 2048 tokens in front of the TripoSG VAE,
 * actionmesh/external/triposg.py:113-151).  Exact greedy FPS, every cloud of the batch on its own, fully determined:
 *
 *   md[i] = +inf for all i;  cur = start_idx[b]
 *   for k in 0 .. n_samples - 1:
 *       out_index[k] = cur;  out_dist[k] = md[cur]             (+inf for k = 0)
 *       d2[i] = ((d0*d0) + (d1*d1)) + (d2*d2) + ...            dc = p[i][c] - p[cur][c] in fp32, left to right over the first
 *                                                              dist_dims channels, every product and sum rounded on its own
 *                                                              (no fma contraction)
 *       md[i] = min(md[i], d2[i])
 *       cur   = the LOWEST index i with md[i] == max(md)
 *
 * 16-bit inputs are converted to fp32 first (exact).  A chosen point has md == 0, so it is chosen again only when every
 * remaining point coincides with a chosen one; the lowest-index rule then returns index 0 from there on, with out_dist 0.
 * Inputs must be finite; with non-finite inputs the call still terminates with every index inside [0, n_points), nothing more.
 * PyTorch3D is not installable where this was written: that its CUDA kernel breaks ties the same way, and how it draws a
 * random start point, are UNPINNED; the contract above is what the tests hold (against a numpy restatement, bit for bit).
 *
 *   points       device, element (b, i, c) at points[b * batch_stride + i * point_stride + c]: strides in ELEMENTS, channels
 *                contiguous - so x[..., :3] of a (B, N, 6) tensor needs no copy, and equal chunks of one cloud can be passed
 *                as extra batch entries of one launch;
 *   dims         channels a point has (1 .. 8; point_stride >= dims);  dist_dims (1 .. dims): those that enter the distance -
 *                3 for the reference's "fps", dims for "fps_full";
 *   start_idx    device int32[batch], NULL = every cloud starts at 0 (values are clamped into [0, n_points));
 *   out_index    device int32 (batch, n_samples);  out_dist: optional device fp32 (batch, n_samples), NULL = not written;
 *   threads      0 = the library's choice; 256 / 512 / 1024 = workgroup size of the resident form (for benchmarks).
 * One workgroup per cloud.  Up to 8192 points the cloud and md stay in registers for the whole launch (the resident form) and
 * no workspace is needed; beyond that (any n_points < 2^31: the streaming form) md and an fp32 copy of the distance channels
 * live in `workspace` - am_fps_workspace_bytes() bytes of 16-byte aligned device scratch for the same (n_points, batch,
 * dist_dims), 0 for the resident form - and are walked once per step. */
#define AM_FPS_F32 0
#define AM_FPS_F16 1    /* IEEE half */
#define AM_FPS_BF16 2
typedef struct {
  const void* points;
  int32_t dtype;                /* AM_FPS_F32 / AM_FPS_F16 / AM_FPS_BF16 */
  int32_t batch;
  int64_t n_points;
  int32_t dims;
  int32_t dist_dims;
  int64_t batch_stride;
  int64_t point_stride;
  int64_t n_samples;            /* K: 1 .. n_points */
  const int32_t* start_idx;
  int32_t* out_index;
  float* out_dist;
  void* workspace;
  size_t workspace_bytes;
  int32_t threads;
  int32_t reserved;
} am_fps_args;
size_t am_fps_workspace_bytes(int64_t n_points, int batch, int dist_dims);
int am_fps(const am_fps_args* args, void* stream);

/* Image preprocessing in front of the context encoder (INTEGRATION seam S8): the reference's `ImagePreprocessor`
 * (actionmesh/preprocessing/image_processor.py:15-146: validity of the alpha mask, composite on white, bounding box, square padding)
 * and the PIL backend of transformers' `BitImageProcessor` (image_encoder.py:48-51: resize of the shortest edge, centre crop,
 * rescale, normalise), restated as integer / table arithmetic so that the device result is BIT-IDENTICAL to theirs.
 *
 * Alpha statistics (am_image_alpha_stats).  rgba: (n_frames, height, width, 4) uint8, contiguous, 4-byte aligned.  Per frame the
 * eight int32 of out_stats[t] are { count(alpha > 127), min column, min row, max column, max row of alpha > 0, 0, 0, 0 }; a frame
 * without any alpha > 0 has min = INT32_MAX and max = -1.  The entry initialises out_stats itself.  Only integer atomics are used
 * (one add / min / max per workgroup), so the result does not depend on scheduling.  The caller reads these rows on the host and
 * decides (image_processor.py:15-23): a frame is valid when count >= int(H W 0.01) and H W - count >= int(H W 0.01); the bounding
 * box is (x, y, w, h) = (min col, min row, max col - min col + 1, max row - min row + 1); frames share the union box unless cropped
 * independently; with m = max(w, h): pad = int(m * padding_ratio), pad_x = pad + (m - w) / 2, pad_y = pad + (m - h) / 2 (integer
 * division), fill value 255 - so the padded frame is (w + 2 pad_x) x (h + 2 pad_y), which may be off square by one pixel.
 *
 * The virtual source image.  Every entry below reads its input through one description per frame (am_image_frame): the window
 * (x0, y0, w, h) of a stored frame of src_w x src_h pixels, surrounded by pad_x columns and pad_y rows of `fill` on each side.
 * With src_channels == 4 the stored pixel is RGBA and each colour byte c with alpha a reads as composite[c * 256 + a], a 64 KiB
 * table the caller supplies: uint8(float32 expression * 255) of image_processor.py:44-52 evaluated by numpy over all 65536 pairs
 * (it differs from floor of the exact blend in 454 pairs, so it is a table, not a formula).  With src_channels == 3 the stored
 * pixel is RGB and is read as it is.  The padded, composited frames never exist in memory unless am_image_materialize writes them.
 *
 * Resample (am_image_resample): PIL's antialiased bicubic resize of 8-bit images followed by a crop, per frame
 *   in = w + 2 pad (width, height); one 1-D pass from `in` to `out` samples: scale = in / out, fs = max(scale, 1), support = 2 fs;
 *   for output i: c = (i + 0.5) scale, taps j in [max(0, trunc(c - support + 0.5)), min(in, trunc(c + support + 0.5))),
 *   w_j = cubic((j - c + 0.5) / fs) (Keys, a = -0.5) divided by their fp64 sum, k_j = trunc(w_j 2^22 + 0.5 sign(w_j));
 *   output = clip_0^255((2^21 + sum_j k_j p_j) >> 22) in int32 with an arithmetic shift.
 * The horizontal pass runs first into a uint8 image (the workspace), the vertical pass on that image; only the rows and columns the
 * crop window (left, top, out_w, out_h of the resized image) needs are computed.  The tap tables are built by the caller in fp64
 * (they depend on (in, out) only) and live in one int32 array `taps`; a table starts at the frame's htab / vtab offset and is
 *   { in, out, ksize, 0,  (first tap, tap count) x out,  k[out][ksize] }.
 * The vertical pass writes out_u8 (n_frames, out_h, out_w, 3) and / or out_pixels (n_frames, 3, out_h, out_w) fp32 =
 * norm_table[channel * 256 + value]: t[v] = (fp32(v * rescale_factor) - fp32(mean)) / fp32(std), built by the caller.
 * Frames may differ in every field but the output size, and a frame's result does not depend on which other frames share the call.
 *
 * frames / taps are HOST arrays (validated before anything is launched: every window inside its frame, every tap inside its image,
 * every offset inside its buffer); frames_dev / taps_dev are the caller's device copies of the same bytes, which the kernels read.
 * Launches only: no allocation, no copy, no synchronisation.  Two launches per am_image_resample and per am_image_alpha_stats, one
 * per am_image_materialize, whatever n_frames is. */
typedef struct {
  int64_t src_offset;           /* bytes from `src` to the frame's first stored pixel (a multiple of 4) */
  int64_t dst_offset;           /* am_image_materialize: bytes from `out` to the frame's first output pixel (a multiple of 4) */
  int32_t src_w, src_h;         /* stored frame, pixels; rows are src_w * src_channels bytes apart */
  int32_t x0, y0, w, h;         /* window of the stored frame */
  int32_t pad_x, pad_y;         /* columns / rows of `fill` on each side */
  int32_t htab, vtab;           /* offsets (in int32) of the two tap tables in `taps` */
  int32_t left, top;            /* crop origin in the resized image */
  int32_t row_lo, n_rows;       /* rows of the padded image the vertical pass reads: [row_lo, row_lo + n_rows) */
} am_image_frame;

typedef struct {
  const uint8_t* rgba;          /* device (n_frames, height, width, 4) */
  int32_t n_frames, height, width;
  int32_t reserved;
  int32_t* out_stats;           /* device (n_frames, 8) */
} am_image_alpha_stats_args;
int am_image_alpha_stats(const am_image_alpha_stats_args* args, void* stream);

typedef struct {
  const uint8_t* src;           /* device, 4-byte aligned */
  int64_t src_bytes;
  int32_t src_channels;         /* 4: RGBA through `composite`; 3: RGB */
  int32_t fill;                 /* 0 .. 255 */
  const uint8_t* composite;     /* device uint8[65536] (src_channels == 4), else NULL */
  int32_t n_frames;
  int32_t out_w, out_h;         /* size of the crop = of the output */
  int32_t reserved;
  const am_image_frame* frames;      /* host, n_frames */
  const am_image_frame* frames_dev;  /* device copy */
  const int32_t* taps;          /* host */
  const int32_t* taps_dev;      /* device copy */
  int64_t taps_len;             /* int32 entries */
  const float* norm_table;      /* device fp32[3 * 256]; needed with out_pixels */
  float* out_pixels;            /* optional device (n_frames, 3, out_h, out_w) */
  uint8_t* out_u8;              /* optional device (n_frames, out_h, out_w, 3) */
  void* workspace;              /* device, 16-byte aligned, am_image_resample_workspace_bytes(n_frames, max n_rows, out_w) */
  size_t workspace_bytes;
} am_image_resample_args;
size_t am_image_resample_workspace_bytes(int n_frames, int max_rows, int out_w);
int am_image_resample(const am_image_resample_args* args, void* stream);

typedef struct {
  const uint8_t* src;           /* as in am_image_resample_args */
  int64_t src_bytes;
  int32_t src_channels;
  int32_t fill;
  const uint8_t* composite;
  int32_t n_frames;
  int32_t reserved;
  const am_image_frame* frames;      /* host: src_offset, dst_offset, src_w, src_h, x0, y0, w, h, pad_x, pad_y are read */
  const am_image_frame* frames_dev;
  uint8_t* out;                 /* device, 4-byte aligned: frame t is (h + 2 pad_y, w + 2 pad_x, 3) uint8 at dst_offset */
  int64_t out_bytes;
} am_image_materialize_args;
int am_image_materialize(const am_image_materialize_args* args, void* stream);

/* Connected components (INTEGRATION seam S9).  Two entries over one union-find whose root is the SMALLEST index of its component, so
 * every result is fully determined; only integer atomics are used (min on labels, add on sizes and counters) and nothing depends on
 * scheduling.  Launches only: no allocation, no copy, no synchronisation, a number of launches that does not depend on the sizes;
 * no kernel waits for another workgroup (the unions are lock-free atomic-min retries, which end because labels only decrease).
 *
 * Mask refinement: the reference's `refine_mask` (actionmesh/preprocessing/background_removal.py:20-38: cv2's Otsu threshold,
 * skimage.measure.label, skimage.morphology.remove_small_objects), per frame:
 *
 *   h[0..255] = histogram of the frame;  N = height * width                       (threshold == -1; else max_val = threshold)
 *   scale = 1.0 / N;  mu = (sum_i i*h[i]) * scale;  mu1 = q1 = max_sigma = 0;  max_val = 0                      all in fp64
 *   for i in 0 .. 255:
 *       p = h[i]*scale;  mu1 *= q1;  q1 += p;  q2 = 1.0 - q1
 *       if min(q1, q2) < FLT_EPSILON or max(q1, q2) > 1.0 - FLT_EPSILON: continue
 *       mu1 = (mu1 + i*p)/q1;  mu2 = (mu - q1*mu1)/q2
 *       sigma = q1*q2*(mu1 - mu2)*(mu1 - mu2)                                      left to right, no fused multiply-add anywhere
 *       if sigma > max_sigma: max_sigma = sigma; max_val = i
 *   foreground = pixel > max_val                                                   (a constant frame: max_val = 0)
 *   components of the foreground under 8-connectivity (skimage's default in 2-D; its input holds only 0 and 255, so labelling
 *   equal-valued regions is labelling the foreground);  size = pixels of a component
 *   out_mask = foreground and size >= min_size ? 255 : 0                           (remove_small_objects drops size < min_size)
 *
 * The loop restates OpenCV's getThreshVal_Otsu_8u followed by THRESH_BINARY.  OpenCV is not installable where this was written:
 * that cv2.threshold returns this very value for every histogram is UNPINNED; the loop above is the contract, and the tests hold
 * the device to a numpy restatement of it exactly, and the labelling to scipy.ndimage.label bit for bit.
 *
 *   mask        device uint8 (n_frames, height, width), contiguous;  height * width < 2^31 - 1, offsets across frames are 64-bit;
 *   out_mask    device uint8, same shape, values 0 / 255 (may be `mask` itself);
 *   out_labels  optional device int32, same shape: 0 on background, 1 + min(y * width + x) over the pixel's component on foreground
 *               - the components BEFORE small ones are removed;
 *   out_stats   optional device int32 (n_frames, 4) = { threshold used, foreground pixels, components, components kept };
 *   workspace   16-byte aligned device scratch of the workspace function's size for the same (n_frames, height, width).
 * A frame's result does not depend on which frames share the call.
 *
 * Graph components: n_nodes nodes and an explicit undirected edge list (self-loops and duplicates allowed, n_edges may be 0).
 *   edges       device int32 (n_edges, 2);
 *   out_label   device int32[n_nodes]: the smallest node index of the node's component;
 *   out_size    optional device int32[n_nodes]: the size of the node's component, written at every node;
 *   out_flag    device int32[1]: 0, or 1 when an edge names a node outside [0, n_nodes) - such an edge is skipped (never
 *               dereferenced) and the caller, who reads the flag together with the result, treats the call as failed. */
typedef struct {
  const uint8_t* mask;
  int32_t n_frames, height, width;
  int32_t min_size;             /* >= 0 */
  int32_t threshold;            /* -1: Otsu per frame; 0 .. 255: that value for every frame */
  int32_t reserved;
  uint8_t* out_mask;
  int32_t* out_labels;
  int32_t* out_stats;
  void* workspace;
  size_t workspace_bytes;
} am_mask_refine_args;
size_t am_mask_refine_workspace_bytes(int n_frames, int height, int width);
int am_mask_refine(const am_mask_refine_args* args, void* stream);

typedef struct {
  int64_t n_nodes;              /* 1 .. 2^31 - 2 */
  int64_t n_edges;
  const int32_t* edges;
  int32_t* out_label;
  int32_t* out_size;
  int32_t* out_flag;
  void* workspace;              /* device, 16-byte aligned, am_graph_components_workspace_bytes(n_nodes, n_edges) */
  size_t workspace_bytes;
} am_graph_args;
size_t am_graph_components_workspace_bytes(int64_t n_nodes, int64_t n_edges);
int am_graph_components(const am_graph_args* args, void* stream);

/* Anchor-mesh preparation (INTEGRATION seam S10): the geometry behind the reference's `get_mesh_features` and `sample_surface`
 * (actionmesh/preprocessing/mesh_processor.py:85-101, 245-285), which go through trimesh's `vertex_normals`, `area_faces`,
 * `face_normals` and `sample.sample_surface`.  ALL geometry is fp64, every operation below rounded on its own in the order written
 * (no fused multiply-add anywhere); a sum of three terms is (x + y) + z.  Vertices are fp32 or fp64 (vertices_f64 = 0 / 1; fp32 is
 * widened first, exact), faces are int32 (n_faces, 3).  n_vertices, n_faces and n_samples are at most (2^31 - 1) / 3.
 *
 * Per face (v0, v1, v2 its three vertices):
 *   e1 = v1 - v0;  e2 = v2 - v0;  c = e1 x e2 = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x);  |c| = sqrt(c . c)
 *   unit face normal = c / |c| (three divisions), or (0, 0, 0) when |c| <= AM_MESH_ZERO;   area = |c| / 2
 *   corner angles (trimesh.triangles.angles):  u = e1 / |e1|;  v = e2 / |e2|;  w = (v2 - v1) / |v2 - v1|
 *     a0 = acos(clip(u . v, -1, 1));  a1 = acos(clip(-(u . w), -1, 1));  a2 = (pi - a0) - a1;   all three 0 for a zero-normal face
 * AM_MESH_ZERO is a recollection of trimesh's `tol.zero` (trimesh is not installable where this was written: UNPINNED).
 *
 * Vertex normals (am_vertex_normals), for n_frames frames that share one topology.  The caller supplies the vertex -> corner CSR
 * of the faces: corner id = 3 * face + k names vertex faces[face][k]; the corners of vertex v are corners[offsets[v] ..
 * offsets[v + 1]), in ASCENDING corner id (one stable sort of the flattened faces).  Per frame and vertex:
 *   s = (0, 0, 0);  for each corner in that order:  s = s + angle[corner] * unit face normal[corner / 3]       (per component)
 *   n = s / |s| (three divisions), or (0, 0, 0) when |s| <= AM_MESH_ZERO;  n32 = fp32(n)
 *   normal = n32 / max(sqrtf((n32x n32x + n32y n32y) + n32z n32z), 1e-12f)                 in fp32: the reference's F.normalize
 * A vertex of valence 0, or one that only zero-normal faces touch, gets exactly (0, 0, 0).  The sum is a gather in CSR order:
 * no floating-point atomics, the same two launches (behind a 4-byte memset of the flag) whatever the valences are, so the result
 * is the same bits on every run.
 *   vertices          device, frame t vertex i component c at vertices[t * frame_stride + 3 * i + c] (stride in ELEMENTS,
 *                     >= 3 * n_vertices; ignored with one frame);
 *   offsets, corners  device int32[n_vertices + 1], int32[3 * n_faces];
 *   out_features      optional device fp32 (n_frames, n_vertices, 6) = position rounded to fp32 | normal;
 *   out_normals       optional device fp32 (n_frames, n_vertices, 3);
 *   out_face_normals  optional device fp64 (n_frames, n_faces, 3): the unit face normals;       at least one output is required
 *   out_flag          device int32[1]: 0, or AM_MESH_BAD_FACE when a face names a vertex outside [0, n_vertices), AM_MESH_BAD_CSR
 *                     when the CSR is not one of these faces (offsets not ascending inside [0, 3 n_faces], a corner outside
 *                     [0, 3 n_faces) or one that does not name the vertex it is listed under).  Every index is compared with its
 *                     bound BEFORE it is used as an address: a bad face contributes zeros, a bad corner nothing, and the caller,
 *                     who reads the flag together with the result, treats the call as failed;
 *   workspace         16-byte aligned device scratch of am_vertex_normals_workspace_bytes(n_frames, n_faces) bytes.
 *
 * Face areas (am_face_areas): out_areas[f] = |c| / 2 as fp64; out_flag as above (AM_MESH_BAD_FACE; such a face gets area 0).
 *
 * Surface samples (am_surface_sample): trimesh.sample.sample_surface with the random draws supplied by the caller.
 *   cdf       device fp64[n_faces]: the inclusive prefix sum of the face areas (the caller's: any non-decreasing weights do);
 *   u_face    device fp64[n_samples] in [0, 1);   u_bary: device fp64 (n_samples, 2) in [0, 1).  Per sample:
 *   pick = u_face * cdf[n_faces - 1];  face = the first index with cdf[face] >= pick        (np.searchsorted, side left; the last
 *                                                                                            face if there is none)
 *   (r0, r1) = u_bary;  if r0 + r1 > 1: r0 = r0 - 1, r1 = r1 - 1;  r0 = |r0|, r1 = |r1|
 *   point = (v0 + (v1 - v0) * r0) + (v2 - v0) * r1                                           per component
 *   out_points      device fp64 (n_samples, 3);   out_face_index: device int32[n_samples];
 *   out_normals     optional device fp64 (n_samples, 3): the unit face normal of the picked face as defined above;
 *   out_flag        as above (AM_MESH_BAD_FACE): the sample of a face with a bad index is (0, 0, 0).
 * A face of zero area has cdf[face] == cdf[face - 1] and is never picked (face 0 is picked by pick == 0 whatever its area).
 * That trimesh draws and combines its uniforms this way is a recollection, UNPINNED; the tests hold the device to a numpy
 * restatement of the lines above: points and face indices exactly, the normals to the rounding of sqrt and acos. */
#define AM_MESH_ZERO 1e-13
#define AM_MESH_BAD_FACE 1
#define AM_MESH_BAD_CSR 2
typedef struct {
  const void* vertices;
  int32_t vertices_f64;         /* 0: fp32, 1: fp64 */
  int32_t n_frames;             /* 1 .. 65535 */
  int64_t n_vertices;
  int64_t n_faces;              /* may be 0: every normal is zero */
  int64_t frame_stride;
  const int32_t* faces;
  const int32_t* offsets;
  const int32_t* corners;
  float* out_features;
  float* out_normals;
  double* out_face_normals;
  int32_t* out_flag;
  void* workspace;
  size_t workspace_bytes;
} am_vertex_normals_args;
size_t am_vertex_normals_workspace_bytes(int n_frames, int64_t n_faces);
int am_vertex_normals(const am_vertex_normals_args* args, void* stream);

typedef struct {
  const void* vertices;         /* one frame, contiguous (n_vertices, 3) */
  int32_t vertices_f64;
  int32_t reserved;
  int64_t n_vertices;
  int64_t n_faces;              /* >= 1 */
  const int32_t* faces;
  double* out_areas;
  int32_t* out_flag;
} am_face_areas_args;
int am_face_areas(const am_face_areas_args* args, void* stream);

typedef struct {
  const void* vertices;         /* one frame, contiguous (n_vertices, 3) */
  int32_t vertices_f64;
  int32_t reserved;
  int64_t n_vertices;
  int64_t n_faces;              /* >= 1 */
  int64_t n_samples;            /* >= 1 */
  const int32_t* faces;
  const double* cdf;
  const double* u_face;
  const double* u_bary;
  double* out_points;
  int32_t* out_face_index;
  double* out_normals;
  int32_t* out_flag;
} am_surface_sample_args;
int am_surface_sample(const am_surface_sample_args* args, void* stream);

/* Mesh decimation (INTEGRATION seam S10): the four kernels behind one ROUND of the parallel quadric edge collapse of
 * actionmesh_amd/mesh_decimate.py, which stands in for the reference's `trimesh.simplify_quadric_decimation`
 * (mesh_processor.py:128-161).  The round loop, the sorts and the compaction are the caller's; a round is
 *   edge evaluation (am_decimate_edges) -> selection of an independent set (am_decimate_select) -> apply (am_decimate_apply),
 * behind am_decimate_quadrics once per mesh.  ALL arithmetic is fp64, every operation rounded on its own in the order written (no
 * fused multiply-add), a sum of three terms is (x + y) + z, a dot product is (ax bx + ay by) + az bz, a cross product
 * a x b = (ay bz - az by, az bx - ax bz, ax by - ay bx).  There are no floating-point atomics: the result is the same bits on every
 * run, and a numpy restatement of the lines below reproduces it bit for bit (tests/test_mesh_decimate_*).
 *
 * Tables the caller supplies (device, int32 unless noted; n_vertices, n_faces <= (2^31 - 1) / 3, n_edges <= 2^31 - 1):
 *   positions  fp64 (n_vertices, 3);   quadrics fp64 (n_vertices, 10);   faces (n_faces, 3), the LIVE faces;
 *   offsets, corners   the vertex -> corner CSR of `faces` as am_vertex_normals defines it (ascending corner id);
 *   edges      (n_edges, 2): the unique undirected edges { u, v } of the faces with u < v (a face with a repeated index may give
 *              u == v: such an edge is never a candidate);
 *   half_edge_to_edge  [3 n_faces]: half-edge 3 f + k runs from faces[f][k] to faces[f][(k + 1) % 3]; the entry is the index of its
 *              undirected edge;
 *   edge_count [n_edges]: how many half-edges map to the edge.
 *
 * A quadric is the symmetric 4 x 4 matrix of a weighted squared plane distance, stored as its upper triangle
 *   q = { xx, xy, xz, xw, yy, yz, yw, zz, zw, ww },   indices (0,0) (0,1) (0,2) (0,3) (1,1) (1,2) (1,3) (2,2) (2,3) (3,3).
 * am_decimate_quadrics, per vertex:  Q = 0;  for each corner of the vertex in CSR order, with (p0, p1, p2) the vertices of its face
 * in face order:
 *   c = (p1 - p0) x (p2 - p0);  len = sqrt(c . c);  a face with len <= AM_MESH_ZERO adds nothing;  n = c / len (three divisions)
 *   d = -(n . p0);  w = len / 2;  p = (nx, ny, nz, d);  Q[i,j] = Q[i,j] + (w * p[i]) * p[j]     for the ten (i, j) in the order above.
 * Quadrics are never recomputed: a collapse u <- v sets Q_u = Q_u + Q_v, element by element.
 *
 * am_decimate_edges, per edge e = (u, v).  `neighbours of s` are the other two vertices of every face of s; the `apexes` a0, a1
 * are the third vertices of the faces that hold both u and v.  The edge passes the TOPOLOGY tests when all of these hold:
 *   lock   u < v, edge_count[e] == 2, and every edge of every face of u and of v that touches u respectively v (the half-edges
 *          3 f + k and 3 f + (k + 2) % 3 of a corner 3 f + k) has edge_count == 2: a vertex on a border or on a non-manifold edge is
 *          never moved or removed;
 *   link   exactly two faces hold both u and v, a0 != a1, neither apex is u or v; over the corners of u, the neighbours w != v that
 *          are also neighbours of v number exactly 4 (each shared neighbour is met twice, so: the apexes and nobody else); both
 *          apexes have valence offsets[a + 1] - offsets[a] > 3; and no OTHER face of u or v holds both apexes.
 * An edge that fails them gets out_positions = (0, 0, 0), out_cost = 0 and the key AM_DECIMATE_NO_KEY.  Otherwise, with
 * Q = Q_u + Q_v (ten additions), pu, pv the endpoints, mid = (pu + pv) * 0.5 per component, E = pv - pu:
 *   the 3 x 3 block and right-hand side:  a = Q0, b = Q1, c = Q2, d = Q4, e = Q5, f = Q7;  r = (-Q3, -Q6, -Q8)
 *   m0 = d f - e e;  m1 = b f - e c;  m2 = b e - d c;  det = (a m0 - b m1) + c m2;   s = r1 f - e r2;  t = r1 e - d r2;  g = b r2 - r1 c
 *   dx = (r0 m0 - b s) + c t;   dy = (a s - r0 m1) + c g;   dz = (a (d r2 - r1 e) - b g) + r0 m2;   x = (dx, dy, dz) / det
 *   conditioning rule (scale-free):  tr = (a + d) + f;  the solve is used only when |det| > AM_DECIMATE_COND * ((tr tr) tr)
 *   and (x - mid) . (x - mid) <= AM_DECIMATE_REACH * (E . E)        (a NaN fails the comparison: within two edge lengths of mid)
 *   cost(y) = ((r0 y0 + r1 y1) + r2 y2) + r3,  r_i = ((Q[i,0] y0 + Q[i,1] y1) + Q[i,2] y2) + Q[i,3]          (y^T Q y, y = (y0 y1 y2 1))
 *   otherwise x = pu, replaced by pv when cost(pv) < cost(x), then by mid when cost(mid) < cost(x)      (ties: u, v, mid)
 *   out_cost = cost(x) when that is > 0, else 0.
 *   no flip: for every face of u without v, and of v without u, with (p0, p1, p2) its vertices in face order and (p0', p1', p2')
 *   the same with the endpoint replaced by x:  c0 = (p1 - p0) x (p2 - p0), c1 likewise;  the edge survives only when
 *   c0 . c1 > (AM_DECIMATE_FLIP * sqrt(c0 . c0)) * sqrt(c1 . c1) for each of them (a degenerate old or new face fails it).
 *   out_key = (uint32 bits of (float)out_cost) << 32 | mix32(e) as int64 when the edge survives, else AM_DECIMATE_NO_KEY (the
 *   position and cost stay).  The fp32 bits of a non-negative number order as the number does, and
 *   mix32(h):     h ^= h >> 16;  h *= 0x85ebca6b;  h ^= h >> 13;  h *= 0xc2b2ae35;  h ^= h >> 16                (uint32, wrapping)
 *   is a bijection, so keys are unique; the hash keeps equal costs (flat regions, regular tessellations) from ordering the
 *   selection along the edge numbering.
 *
 * am_decimate_select (three launches, gathers only):  m1[v] = min key over the edges that touch v (NO_KEY without one);
 *   m2[v] = min(m1[v], m1[w]) over the neighbours w of v;   out_selected[e] = 1 when key[e] != NO_KEY and key[e] == m2[u] == m2[v],
 *   else 0.  Endpoints of two selected edges are neither equal nor adjacent, so their closed stars share no face.
 *
 * am_decimate_apply, per kept edge index kept[i] = e = (u, v), for a caller-chosen SUBSET of the selected edges: positions[u] =
 *   candidate[e];  quadrics[u] = quadrics[u] + quadrics[v];  every face of v that also holds u gets out_face_dead = 1, in every
 *   other face of v the corner v becomes u;  vertex_map[v] = u.  positions, quadrics, faces and vertex_map are updated in place;
 *   out_face_dead is cleared first.  Edges that were not selected together may race: that is the caller's responsibility, but no
 *   index is used unchecked.
 *
 * out_flag, device int32[1], cleared by each call; the caller reads it with the result and treats a non-zero value as failure:
 *   AM_DECIMATE_BAD_FACE  a face names a vertex outside [0, n_vertices);
 *   AM_DECIMATE_BAD_CSR   offsets not ascending inside [0, 3 n_faces], a corner outside [0, 3 n_faces) or one that does not name the
 *                         vertex it is listed under;
 *   AM_DECIMATE_BAD_EDGE  an edge endpoint outside [0, n_vertices) or u > v, a half_edge_to_edge entry outside [0, n_edges) or one
 *                         whose edge is not that half-edge's;
 *   AM_DECIMATE_BAD_KEPT  a kept index outside [0, n_edges).
 * Every index read from memory is compared with its bound BEFORE it is used as an address; what a bad index would have
 * contributed is left out. */
#define AM_DECIMATE_COND 1e-10
#define AM_DECIMATE_REACH 4.0
#define AM_DECIMATE_FLIP 0.2
#define AM_DECIMATE_NO_KEY INT64_MAX
#define AM_DECIMATE_BAD_FACE AM_MESH_BAD_FACE      /* the same two conditions, found by the same device code */
#define AM_DECIMATE_BAD_CSR AM_MESH_BAD_CSR
#define AM_DECIMATE_BAD_EDGE 4
#define AM_DECIMATE_BAD_KEPT 8
typedef struct {
  const double* positions;
  int64_t n_vertices;           /* >= 1 */
  int64_t n_faces;              /* >= 1 */
  const int32_t* faces;
  const int32_t* offsets;
  const int32_t* corners;
  double* out_quadrics;         /* (n_vertices, 10) */
  int32_t* out_flag;
} am_decimate_quadrics_args;
int am_decimate_quadrics(const am_decimate_quadrics_args* args, void* stream);

typedef struct {
  const double* positions;
  const double* quadrics;
  int64_t n_vertices;
  int64_t n_faces;
  int64_t n_edges;              /* >= 1 */
  const int32_t* faces;
  const int32_t* offsets;
  const int32_t* corners;
  const int32_t* edges;
  const int32_t* half_edge_to_edge;
  const int32_t* edge_count;
  double* out_positions;        /* (n_edges, 3) */
  double* out_cost;             /* [n_edges] */
  int64_t* out_key;             /* [n_edges] */
  int32_t* out_flag;
} am_decimate_edges_args;
int am_decimate_edges(const am_decimate_edges_args* args, void* stream);

typedef struct {
  int64_t n_vertices;
  int64_t n_faces;
  int64_t n_edges;
  const int32_t* faces;
  const int32_t* offsets;
  const int32_t* corners;
  const int32_t* edges;
  const int32_t* half_edge_to_edge;
  const int64_t* keys;
  int64_t* out_m1;              /* [n_vertices] */
  int64_t* out_m2;              /* [n_vertices] */
  uint8_t* out_selected;        /* [n_edges] */
  int32_t* out_flag;
} am_decimate_select_args;
int am_decimate_select(const am_decimate_select_args* args, void* stream);

typedef struct {
  int64_t n_vertices;
  int64_t n_faces;
  int64_t n_edges;
  int64_t n_kept;               /* >= 1 */
  const int32_t* kept;          /* [n_kept] edge indices */
  const int32_t* edges;
  const double* candidates;     /* (n_edges, 3): am_decimate_edges' out_positions */
  const int32_t* offsets;
  const int32_t* corners;
  double* positions;            /* in place */
  double* quadrics;             /* in place */
  int32_t* faces;               /* in place */
  int32_t* vertex_map;          /* [n_vertices], in place */
  uint8_t* out_face_dead;       /* [n_faces] */
  int32_t* out_flag;
} am_decimate_apply_args;
int am_decimate_apply(const am_decimate_apply_args* args, void* stream);

/* Border collapses (`borders="collapse"` of mesh_decimate.py): am_decimate_border_quadrics and am_decimate_border_edges take the
 * places of am_decimate_quadrics and am_decimate_edges in the round above; am_decimate_select and am_decimate_apply serve as they
 * are (the selection's independence does not depend on borders, and apply marks dead exactly the faces of v that hold u: two for an
 * interior edge, one for a border edge).  Tables, arithmetic rules, flag bits and the restatement (tests/_decimate_border_ref.py,
 * tests/test_mesh_decimate_border_*) are those of the text above.  On a mesh without border every output equals the old kernels' bits.
 *
 * VERTEX CLASSES, from edge_count over the half-edges 3 f + k and 3 f + (k + 2) % 3 of every corner 3 f + k of the vertex (an edge
 * of count 2 is met twice, one of count 1 once):
 *   interior  every such count is 2;
 *   border    every such count is 1 or 2, and exactly two of them are 1;
 *   locked    anything else: a count above 2, or a number of count-1 edges other than 0 or 2.  Never moved or removed.
 *
 * TOPOLOGY, the rule.  Close the surface with a cone: one imaginary vertex W and one imaginary face (q, p, W) for every half-edge
 * p -> q of count 1.  In that complex the `opposite` vertices of an edge { u, v } are the third vertices of its faces: two real
 * apexes for an edge of count 2, one real apex and W for an edge of count 1.  An edge with u < v, edge_count 1 or 2 and two
 * endpoints that are not locked passes when, in the coned complex,
 *   (a) the common neighbours of u and v are exactly the opposite vertices, and those two differ (neither is u or v);
 *   (b) no edge lies in the link of u and in the link of v: for the pair { apex, W } that is "the faces (u, apex, W) and (v, apex, W)
 *       do not both exist"; for two real apexes the rule stays today's stricter one, no OTHER face of u or v holds both apexes;
 *   (c) every real apex has coned valence > 3: its face count offsets[a + 1] - offsets[a], plus 2 when it is a border vertex
 *       (a locked apex counts its real faces only);
 *   (d) the merged vertex keeps coned valence > 3: (coned valence of u) + (coned valence of v) - 4 > 3.  Under (a) to (c) this always
 *       holds between two interior vertices (today's (b) never removes a vertex of three faces); on a border it keeps a collapse
 *       from leaving an isolated triangle: the two-triangle strip, whose coned complex is two glued tetrahedra, comes back whole as
 *       that closed mesh does today.
 * The cases that follow, which the kernel carries (n_faces(u, v): the faces of u that hold v; a neighbour w of u is met once per
 * face of u that holds it, so `shared` below weighs a neighbour met through a count-1 edge { u, w } twice):
 *   every edge                               (d), with the endpoints' classes and face counts offsets[s + 1] - offsets[s];
 *   edge_count[e] == 2, u and v interior     today's rule, unchanged: n_faces == 2, shared == 4, (b), (c);
 *   edge_count[e] == 2, one endpoint border  the same tests; the merged vertex is a border vertex;
 *   edge_count[e] == 2, both border          never: W is a common neighbour and not opposite (the collapse would pinch the surface);
 *   edge_count[e] == 1                       n_faces == 1, shared == 2 (the apex and nobody else: on a border loop of three edges
 *                                            the other border neighbours of u and v coincide, are shared and are not the apex),
 *                                            not both { u, apex } and { v, apex } of count 1 (the face would be an isolated
 *                                            triangle), (c).  An ear - a border vertex of one face whose third edge is interior -
 *                                            collapses along either of its border edges and takes its face with it, (d) allowing.
 *   shared = the sum, over the corners of u and over both neighbours w != v of the corner that are also neighbours of v, of
 *            (edge_count{ u, w } == 1 ? 2 : 1).
 * The number of half-edges { u, v } met over the corners of u must equal edge_count[e] (AM_DECIMATE_BAD_EDGE otherwise, and so
 * is a count below 1).
 *
 * am_decimate_border_quadrics, per vertex: Q = 0; for each corner 3 f + k of the vertex in CSR order: FIRST the face's plane exactly
 * as am_decimate_quadrics adds it (a face with len <= AM_MESH_ZERO adds nothing, its border planes included), THEN, for the
 * corner's outgoing half-edge 3 f + k and then its incoming half-edge 3 f + (k + 2) % 3, when that edge has count 1, one constraint
 * plane through the edge and perpendicular to the face.  With n the face's unit normal from above and p -> q the half-edge in face
 * order:
 *   E = q - p;  m = E x n;  ml = sqrt(m . m);  a plane with ml <= AM_MESH_ZERO adds nothing;  m = m / ml (three divisions);
 *   d = -(m . p);  w = border_weight * (E . E);  P = (mx, my, mz, d);  Q[i,j] = Q[i,j] + (w * P[i]) * P[j]   in the order above.
 * border_weight is the caller's, finite and >= 0; mesh_decimate.py's default is 1.0.  The argument for that value, and nothing
 * stronger: a face's plane weighs its area, about 0.43 L^2 for an edge length L, and an interior vertex sums 5 to 6 of them; a
 * border vertex sums two border planes of L^2 each, so leaving the border curve by a distance costs about what leaving the
 * surface by the same distance does.  Quadrics are summed on collapse and never recomputed, as above.
 *
 * am_decimate_border_edges, per edge: an edge that fails the topology gets (0, 0, 0), cost 0 and AM_DECIMATE_NO_KEY.  Otherwise
 * position, cost and key are EXACTLY am_decimate_edges' expressions on Q_u + Q_v: the solve with its conditioning and reach rules,
 * else u, v, mid; the no-flip test over every face of u without v and of v without u; the key.  (Remark, not a rule: on a straight
 * border in a flat region the solve is singular, and the fallback keeps the vertex on the line.)  A collapse removes
 * edge_count[e] faces, 1 or 2. */
typedef struct {
  const double* positions;
  int64_t n_vertices;
  int64_t n_faces;
  int64_t n_edges;              /* >= 1 */
  const int32_t* faces;
  const int32_t* offsets;
  const int32_t* corners;
  const int32_t* half_edge_to_edge;
  const int32_t* edge_count;
  double border_weight;         /* finite, >= 0 */
  double* out_quadrics;         /* (n_vertices, 10) */
  int32_t* out_flag;
} am_decimate_border_quadrics_args;
int am_decimate_border_quadrics(const am_decimate_border_quadrics_args* args, void* stream);

typedef struct {
  const double* positions;
  const double* quadrics;
  int64_t n_vertices;
  int64_t n_faces;
  int64_t n_edges;              /* >= 1 */
  const int32_t* faces;
  const int32_t* offsets;
  const int32_t* corners;
  const int32_t* edges;
  const int32_t* half_edge_to_edge;
  const int32_t* edge_count;
  double* out_positions;        /* (n_edges, 3) */
  double* out_cost;             /* [n_edges] */
  int64_t* out_key;             /* [n_edges] */
  int32_t* out_flag;
} am_decimate_border_edges_args;
int am_decimate_border_edges(const am_decimate_border_edges_args* args, void* stream);

/* Iso-surface extraction (INTEGRATION seam S11): marching tetrahedra on a regular grid, the three kernels behind
 * actionmesh_amd/isosurface.py, which stands in for the `diso` dual marching cubes inside TripoSG's hierarchical_extract_geometry
 * (actionmesh/external/triposg.py:13, 193-199).  The two prefix sums between the kernels, the sizing of the outputs and the removal
 * of unused vertices are the caller's.  There are no atomics but the OR into the flag word and no hash table: the result is the same
 * bits on every run, and a numpy restatement of the lines below reproduces it bit for bit (tests/test_isosurface_*).
 *
 * Grid.  `values` is fp32 (nx, ny, nz), contiguous, every axis >= 2 and nx ny nz <= 2^31 - 1.  Point (i, j, k) has the linear index
 * p = (i ny + j) nz + k and the position origin[c] + idx[c] * spacing[c] per component, fp64, a multiply then an add (no fused
 * multiply-add).  A point is INSIDE when its value is finite and (double)value > level (inside_above != 0) or (double)value < level
 * (inside_above == 0).  A non-finite value means "not evaluated".  The surface is oriented with its normals from the inside to the
 * outside whichever comparison is chosen, so inside_above = 0 gives the reverse winding of inside_above = 1 on the same values - and
 * on the negated values, with the negated level, the identical mesh.
 *
 * Subdivision.  Every cell - eight points p + m, m in {000 .. 111} with bits (di, dj, dk), dk lowest - is cut into the six Kuhn
 * (Freudenthal) tetrahedra.  Tetrahedron t belongs to the t-th permutation pi of the axes (i, j, k) in lexicographic order; its
 * corners are c0 = 000, c1 = c0 + e_pi0, c2 = c1 + e_pi1, c3 = 111.  Every edge of a tetrahedron therefore runs from a grid point p to
 * p + m for one of the seven non-zero offsets m, and face and body diagonals agree between neighbouring cells.
 *
 * Vertices.  Edge (p, m) CROSSES when p + m is inside the grid, both ends are finite and exactly one is inside.  It has the id
 * 7 p + (m - 1); there is one vertex per crossing edge, numbered in ascending id.  With a = p, b = p + m, in fp64:
 *   t = (level - v_a) / (v_b - v_a);   position[c] = pa[c] + t * (pb[c] - pa[c]),   rounded once to fp32.
 *
 * Triangles.  A tetrahedron with a non-finite corner emits nothing.  Otherwise the inside mask of (c0 .. c3), bit q for corner q,
 * selects one of 14 cases; a polygon vertex is the vertex of the edge between two corners:
 *   one inside corner a:     the polygon (a, o) over the outside corners o in ascending order;
 *   three inside corners:    the polygon (i, o) over the inside corners i in ascending order, o the outside one;
 *   two inside corners:      the quad (i0, o0), (i0, o1), (i1, o1), (i1, o0), split along its first and third vertex into
 *                            (q0, q1, q2) and (q0, q2, q3).
 * A polygon is reversed - first vertex kept, the rest in reverse order, BEFORE the split - when its normal
 * (q1 - q0) x (q2 - q0), taken on the unit tetrahedron with the edge midpoints as crossings, has a negative dot product with
 * (mean of the outside corners) - (mean of the inside corners).  Triangles are ordered by the linear index of the cell's 000 corner,
 * then tetrahedron, then triangle; faces are int32.
 *
 * am_iso_classify, per point p:  out_mask[p] = bit (m - 1) for every crossing edge (p, m);  out_count[p] = the number of triangles,
 *   0 .. 12, of the cell whose 000 corner is p, and 0 where no cell starts (i = nx - 1, j = ny - 1 or k = nz - 1).
 * The caller makes the exclusive prefix sums vertex_offset[p] over popcount(out_mask) and tri_offset[p] over out_count (int64); their
 * totals are n_vertices and n_triangles, each 1 .. 2^31 - 1 for the two calls below.
 * am_iso_vertices, per point with a non-zero mask:  the vertex of edge (p, m) goes to row vertex_offset[p] + popcount(mask[p] &
 *   ((1 << (m - 1)) - 1)) of out_vertices (n_vertices, 3) fp32.
 * am_iso_triangles, per point with a non-zero count:  the cell's triangles go to rows tri_offset[p] .. of out_faces (n_triangles, 3);
 *   the vertex of edge (p, m) is vertex_offset[p] + popcount(mask[p] & ((1 << (m - 1)) - 1)).
 *
 * out_flag, device int32[1], cleared by each of the two calls; the caller reads it with the result and treats a non-zero value as
 * failure:
 *   AM_ISO_BAD_VERTEX_OFFSET  a vertex offset is negative or leads past n_vertices;
 *   AM_ISO_BAD_TRI_OFFSET     a triangle offset is negative or leads past n_triangles;
 *   AM_ISO_BAD_TABLE          mask or count do not belong to these values: a mask above 127, a mask bit for an edge that leaves the
 *                             grid or that a triangle needs and the mask lacks, a count above 12, where no cell starts, or other
 *                             than the number of triangles the values give.
 * Every offset and index read from memory is compared with its bound BEFORE it is used as an address; what a bad one would have
 * written is left out. */
#define AM_ISO_BAD_VERTEX_OFFSET 1
#define AM_ISO_BAD_TRI_OFFSET 2
#define AM_ISO_BAD_TABLE 4
typedef struct {
  const float* values;          /* (nx, ny, nz) */
  int64_t nx;
  int64_t ny;
  int64_t nz;
  double level;                 /* finite */
  int32_t inside_above;
  int32_t reserved;
  uint8_t* out_mask;            /* [nx ny nz] */
  uint8_t* out_count;           /* [nx ny nz] */
} am_iso_classify_args;
int am_iso_classify(const am_iso_classify_args* args, void* stream);

typedef struct {
  const float* values;
  int64_t nx;
  int64_t ny;
  int64_t nz;
  double level;
  double origin[3];
  double spacing[3];
  const uint8_t* mask;          /* am_iso_classify's out_mask */
  const int64_t* vertex_offset; /* [nx ny nz] */
  int64_t n_vertices;           /* >= 1 */
  float* out_vertices;          /* (n_vertices, 3) */
  int32_t* out_flag;
} am_iso_vertices_args;
int am_iso_vertices(const am_iso_vertices_args* args, void* stream);

typedef struct {
  const float* values;
  int64_t nx;
  int64_t ny;
  int64_t nz;
  double level;
  int32_t inside_above;
  int32_t reserved;
  const uint8_t* mask;
  const uint8_t* count;         /* am_iso_classify's out_count */
  const int64_t* vertex_offset;
  const int64_t* tri_offset;    /* [nx ny nz] */
  int64_t n_vertices;
  int64_t n_triangles;          /* >= 1 */
  int32_t* out_faces;           /* (n_triangles, 3) */
  int32_t* out_flag;
} am_iso_triangles_args;
int am_iso_triangles(const am_iso_triangles_args* args, void* stream);

/* Iso-surface extraction, the second method (isosurface.py, method="dual"): dual marching cubes with a manifold rule - one vertex per
 * patch of every active cell, one quad per crossing grid edge, about a third of the triangles of am_iso_*.  The four kernels below;
 * the two prefix sums between them, the sizing of the outputs and the removal of unused vertices are the caller's, as for am_iso_*.
 * There are no atomics but the OR into the flag word and no hash table: the result is the same bits on every run, and a numpy
 * restatement of the lines below, which DERIVES the tables the kernels carry as constants, reproduces it bit for bit
 * (tests/test_dualcubes_*).  UNPINNED: parity with `diso` - its vertex placement, its diagonal rule, its tables - and sharp-feature
 * (QEF) placement.
 *
 * Grid.  As for am_iso_*: `values` is fp32 (nx, ny, nz), contiguous, every axis >= 2 and nx ny nz <= 2^31 - 1; point (i, j, k) has the
 * linear index p = (i ny + j) nz + k and the position origin[c] + idx[c] * spacing[c] per component, fp64, a multiply then an add (no
 * fused multiply-add); a point is INSIDE when its value is finite and (double)value > level (inside_above != 0) or (double)value <
 * level (inside_above == 0); a non-finite value means "not evaluated"; the normals point from the inside to the outside whichever
 * comparison is chosen, so the negated values with the negated level and the other comparison give the identical mesh.
 *
 * Cell.  The cell p has the eight points p + m, m in {000 .. 111} with bits (di, dj, dk), dk lowest; it exists when i < nx - 1,
 * j < ny - 1 and k < nz - 1.  It is ACTIVE when all eight values are finite and they are not all on one side.  Its CONFIGURATION is
 * the 8-bit inside mask, bit m for corner m (1 .. 254 on an active cell).  The twelve cell edges are the corner pairs (a, b), a < b,
 * that differ in one bit, numbered 0 .. 11 in ascending (a, b): (0,1) (0,2) (0,4) (1,3) (1,5) (2,3) (2,6) (3,7) (4,5) (4,6) (5,7)
 * (6,7).  A cell edge CROSSES when exactly one of its corners is inside.  Face 2 axis + side (axis 0, 1, 2 = i, j, k) holds the four
 * corners whose bit of that axis equals `side`.
 *
 * Patches.  On each of the six faces, two crossing edges are joined by one segment; a face with four crossing edges (AMBIGUOUS: its
 * diagonal corners are inside) gets two segments, each joining the two face edges at one INSIDE corner of the face (cutting that
 * corner off) - the default rule.  Every crossing edge lies on two faces, so the segments form cycles over the crossing edges; each
 * cycle is a PATCH.  Patches are numbered by their smallest edge id, ascending.  The 256 configurations have 0 / 1 / 2 / 3 / 4
 * patches in 2 / 162 / 82 / 8 / 2 cases.
 *
 * Flip (what makes the mesh a manifold).  An ambiguous face of a cell is DOUBLE when the default rule puts both of its segments on the
 * same patch.  A face shared by two ACTIVE cells is FLIPPED when it is double in both; on a flipped face the two segments cut off the
 * OUTSIDE corners instead, in both cells.  A face on the grid border, or towards a cell that is not active, never flips.  Exactly 36
 * configurations have a double face and each of them has exactly one ambiguous face, so a cell has at most one flipped face, and its
 * state - its CODE - is its configuration, + 256 when that face is flipped (int16; 0 where no active cell starts).
 *
 * Dual vertices.  One per patch of every active cell, numbered by the linear index of the cell's 000 corner, then by patch.  Its
 * position: the crossing positions of the patch's edges (a, b), each with t = (level - v_a) / (v_b - v_a) and, per component,
 * pa[c] + t * (pb[c] - pa[c]) in fp64 as in am_iso_vertices but NOT rounded to fp32, are added in ascending edge id to a sum that
 * starts at +0, the sum is divided by their number, and the quotient is rounded once to fp32.
 *
 * Quads and triangles.  The grid edge (p, axis) from p to p + e_axis EMITS when the four cells around it - p, p - e_u, p - e_u - e_v,
 * p - e_v with u = (axis + 1) mod 3, v = (axis + 2) mod 3 - all exist and are ACTIVE, and it crosses.  Its quad (q0, q1, q2, q3) has,
 * in that order of the cells, the vertex of the patch that holds this edge in each cell; when p is not inside (the far end is), q1 and
 * q3 change places, so that the normal points from the inside to the outside.  The quad is split along its shorter diagonal: with
 * d02 = |q0 - q2|^2 and d13 = |q1 - q3|^2 - each ((x x + y y) + z z) in fp64 on the differences of the STORED fp32 positions - the
 * triangles are (q0, q1, q3), (q1, q2, q3) when d13 < d02 and (q0, q1, q2), (q0, q2, q3) otherwise (a tie goes to first - third).
 * Triangles are ordered by 3 p + axis, two per quad; faces are int32.
 *
 * am_dmc_cells, per point p:  out_config[p] = the configuration of the cell p when it is ACTIVE, 0 otherwise and where no cell starts;
 *   out_double[p] = the 6-bit mask of that configuration's double faces, bit 2 axis + side (0 or one bit).
 * am_dmc_classify, per point p, from the two results above:  out_code[p];  out_count[p] = the cell's number of patches, 0 .. 4, under
 *   that code;  out_edge_mask[p] = bit `axis` for every emitting edge (p, axis).
 * The caller makes the exclusive prefix sums vertex_offset[p] over out_count and tri_offset[p] over 2 popcount(out_edge_mask) (int64);
 * their totals are n_vertices and n_triangles, each 1 .. 2^31 - 1 for the two calls below.
 * am_dmc_vertices, per point with a non-zero code:  the vertex of patch q goes to row vertex_offset[p] + q of out_vertices.
 * am_dmc_triangles, per point with a non-zero edge mask:  the two triangles of edge (p, axis) go to rows tri_offset[p] +
 *   2 popcount(edge_mask[p] & ((1 << axis) - 1)) and the next of out_faces; the vertex of patch q of cell c is vertex_offset[c] + q;
 *   `vertices` is am_dmc_vertices' output (the diagonals).  Dual vertices that no quad uses - next to non-finite samples or to the grid
 *   border - stay in out_vertices; the caller drops them, order preserved.
 *
 * out_flag, device int32[1], cleared by each of the last two calls; the caller reads it with the result and treats a non-zero value
 * as failure:
 *   AM_DMC_BAD_VERTEX_OFFSET  a vertex offset is negative or leads past n_vertices;
 *   AM_DMC_BAD_TRI_OFFSET     a triangle offset is negative or leads past n_triangles;
 *   AM_DMC_BAD_CODE           code or edge mask do not belong to these values: a code outside 0 .. 511, with the configuration 0 or
 *                             255, with + 256 on a configuration without a double face, where no cell starts, or (am_dmc_vertices)
 *                             with another configuration than the values give; an edge mask above 7, a mask bit where one of the
 *                             four cells does not exist or has the code 0, or for an edge that does not cross under the cell's code.
 * Every offset, code and index read from memory is compared with its bound BEFORE it is used as an address; what a bad one would have
 * written is left out. */
#define AM_DMC_BAD_VERTEX_OFFSET 1
#define AM_DMC_BAD_TRI_OFFSET 2
#define AM_DMC_BAD_CODE 4
typedef struct {
  const float* values;          /* (nx, ny, nz) */
  int64_t nx;
  int64_t ny;
  int64_t nz;
  double level;                 /* finite */
  int32_t inside_above;
  int32_t reserved;
  uint8_t* out_config;          /* [nx ny nz] */
  uint8_t* out_double;          /* [nx ny nz] */
} am_dmc_cells_args;
int am_dmc_cells(const am_dmc_cells_args* args, void* stream);

typedef struct {
  int64_t nx;
  int64_t ny;
  int64_t nz;
  const uint8_t* config;        /* am_dmc_cells' out_config */
  const uint8_t* double_faces;  /* am_dmc_cells' out_double */
  int16_t* out_code;            /* [nx ny nz] */
  uint8_t* out_count;           /* [nx ny nz] */
  uint8_t* out_edge_mask;       /* [nx ny nz] */
} am_dmc_classify_args;
int am_dmc_classify(const am_dmc_classify_args* args, void* stream);

typedef struct {
  const float* values;
  int64_t nx;
  int64_t ny;
  int64_t nz;
  double level;
  double origin[3];
  double spacing[3];
  int32_t inside_above;
  int32_t reserved;
  const int16_t* code;          /* am_dmc_classify's out_code */
  const int64_t* vertex_offset; /* [nx ny nz] */
  int64_t n_vertices;           /* >= 1 */
  float* out_vertices;          /* (n_vertices, 3) */
  int32_t* out_flag;
} am_dmc_vertices_args;
int am_dmc_vertices(const am_dmc_vertices_args* args, void* stream);

typedef struct {
  int64_t nx;
  int64_t ny;
  int64_t nz;
  const int16_t* code;
  const uint8_t* edge_mask;     /* am_dmc_classify's out_edge_mask */
  const int64_t* vertex_offset;
  const int64_t* tri_offset;    /* [nx ny nz] */
  const float* vertices;        /* am_dmc_vertices' out_vertices */
  int64_t n_vertices;
  int64_t n_triangles;          /* >= 1 */
  int32_t* out_faces;           /* (n_triangles, 3) */
  int32_t* out_flag;
} am_dmc_triangles_args;
int am_dmc_triangles(const am_dmc_triangles_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ACTIONMESH_AMD_H */
