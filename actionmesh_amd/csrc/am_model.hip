// Model-level orchestration of the Stage-I denoiser forward on one MI355X:
// weights resident in HBM (bf16 matrices, fp32 norm/bias vectors), every
// activation buffer pre-allocated for the bound problem size, and the forward
// issued as a fixed sequence of the kernels in this library on the caller's
// stream.  Mirrors ActionMeshDenoiser.forward (temporal_denoiser.py:151-249)
// and FlowMatchingBlock.forward (block.py:110-154); the cross-attention K/V of
// the step-invariant context are cached per window (am_set_context).
#include <vector>

#include <stdlib.h>
#include <string.h>

#include "am_common.h"

int am_add_bias_rows(bf16_t* h, const float* bias, int64_t rows, int C, void* stream);    // am_elementwise.hip
int am_add_bias_rows_stats(bf16_t* h, const float* bias, int64_t rows, int C, float eps, float* stats, void* stream);   // am_norm.hip

// diagnostic trace point (am_common.h am_trace): a checksum of `bytes` at `ptr` behind the kernel that has just been enqueued
#define TR(stage, layer, ptr, bytes) do { if (am_trace_on()) am_trace((stage) * 100 + (layer), (ptr), (size_t)(bytes), (void*)st); } while (0)

namespace {
constexpr int HD = 128;                                 // head dimension
constexpr float LN_EPS = 1e-5f, QK_EPS = 1e-6f;         // LayerNorm / qk-RMSNorm
constexpr float SOFTMAX_SCALE = 0.08838834764831845f;   // 1/sqrt(128)
inline int pad_to(int64_t x, int m) { return (int)round_up(x, m); }
}  // namespace

// A linear [N][C] that sits behind a LayerNorm (block.py:138 norm_s_attn -> to_q|k|v, :146 norm_x_attn -> to_q, :152 norm_ff -> ff.net.0,
// temporal_denoiser.py:239-242 norm_out -> proj_out): the loaded operands, and the norm folded in (am_ln_fold_weight): wf = W (.) gamma,
// its column sums cs, and d = W beta + bias
struct am_folded {
  bf16_t* w = nullptr;
  float *bias = nullptr, *ln_w = nullptr, *ln_b = nullptr;
  bf16_t* wf = nullptr;
  float *cs = nullptr, *d = nullptr;
  int N = 0;
};

struct am_layer {
  am_folded qkv, xq, ff1;
  bf16_t *w_so = nullptr, *w_xkv = nullptr, *w_xo = nullptr, *w_ff2 = nullptr, *w_skip = nullptr;
  float *b_so = nullptr, *b_xo = nullptr, *b_ff2 = nullptr, *b_skip = nullptr, *ln_k_w = nullptr, *ln_k_b = nullptr;
  float *s_nq = nullptr, *s_nk = nullptr, *x_nq = nullptr, *x_nk = nullptr;
  bf16_t *kx = nullptr, *vtx = nullptr;   // cross-attention K / V^T cache
};

struct am_model {
  am_config cfg;
  int C, H, F, Dc, Din, NL, P, rank;
  std::vector<am_layer> layers;
  bf16_t *w_t1 = nullptr, *w_t2 = nullptr, *w_in = nullptr;
  float *b_t1 = nullptr, *b_t2 = nullptr, *b_in = nullptr;
  am_folded out;
  std::vector<uint8_t> loaded;                  // per (layer + 1, row of the weight table): the key has been loaded
  int n_expected = 0;                           // keys of the weight table that exist for this configuration
  std::vector<void*> allocs;
  float* stage_f32 = nullptr;
  size_t stage_elems = 0;
  // Host arguments are BORROWED for the call only (header conventions), but an asynchronous copy from pageable memory may run
  // after the call has returned - the caller's array can be gone by then (a ctypes temporary is freed at once; seen as one
  // garbage per-frame diffusion time in a forward when the device was busy).  Host data is therefore copied into a pinned
  // ring slot owned by the handle before the asynchronous copy is queued; a slot is re-used only after its copy has executed.
  // am_denoise_forward_graph: one captured forward per (operands, shape, stream, window) key
  struct GraphCache {
    const float* x = nullptr; uint16_t* v = nullptr; int B = 0, T = 0, N = 0; hipStream_t st = nullptr; uint64_t ctx_gen = 0, scratch_gen = 0;
    bool warm = false, disabled = false;
    hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
    uint64_t replays = 0, captures = 0, eager = 0;
  } gc;
  uint64_t ctx_gen = 0;        // bumped by everything a captured forward bakes in (context, hints, K/V buffers)
  struct HostStage { void* pinned = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool used = false; };
  HostStage hstage[8];
  unsigned hstage_next = 0;

  // workspace
  int maxB, maxT, maxN, maxS, maxL;
  int64_t maxR;
  bf16_t *hwork = nullptr, *z = nullptr, *ao = nullptr, *qkv = nullptr, *ffh = nullptr;
  std::vector<bf16_t*> skip;
  bf16_t *Qb = nullptr, *Kg = nullptr, *Vtg = nullptr;
  uint8_t *Q8 = nullptr, *K8 = nullptr, *Vt8 = nullptr;   // fp8 operand copies (cfg.attn_fp8); K8 / Vt8 = the gather buffers when P > 1
  bool kv8_external = false;
  size_t chunk_stride8 = 0;    // bytes between consecutive ranks' K8 (or Vt8) chunks
  uint64_t n_attn_fp8 = 0, n_attn_bf16 = 0;   // inflated self-attention launches by arithmetic type (am_attention_counters)
  bool kv_external = false;
  size_t chunk_elems = 0;
  size_t chunk_stride = 0;     // elements between consecutive ranks' K (or V^T) chunks
  float* attn_state = nullptr; // two-pass self-attention: (O, m, l) of every query row after the local K/V shard
  bool local_done = false;     // am_layer_attn_local ran for the layer in flight
  bf16_t *xb = nullptr, *te0 = nullptr, *te1 = nullptr, *ctxb = nullptr, *kvtmp = nullptr;
  float *tdev = nullptr, *rope_cos = nullptr, *rope_sin = nullptr;
  // Folded LayerNorms: norm_s_attn / norm_x_attn / norm_ff are never launched and their outputs never exist in HBM.
  // INVARIANT while ln_fold is on: between the kernels of a forward, ln_stats[r] = (mean, rstd) of row r of the current residual
  // stream buffer (h->hsrc / h->hwork) - written by whoever wrote the rows: the producer GEMM's store loop through ln_part +
  // am_row_stats_finalize, the norm_skip LayerNorm, or am_row_stats_bf16 for rows no GEMM produced.
  bool ln_fold = true, folds_ready = false, ln_recompute = false;
  float *ln_stats = nullptr, *ln_part = nullptr;

  // per-window / per-forward state
  std::vector<uint8_t> ctx_zero;   // am_set_branch_hints: batch rows whose context is identically zero
  bool shared_prefix = false;      // am_set_branch_hints: all batch rows share hidden_states and t_bt
  bool ctx_set = false;
  int ctxB = 0, ctxT = 0, ctxS = 0;
  bool in_forward = false;
  int B = 0, T = 0, N = 0, L = 0;
  int64_t R = 0;
  bf16_t* hsrc = nullptr;
  int skip_top = 0;
  int next_layer = 0;   // enforces pre/post call order
  bool pre_done = false;

  bool inflated(int i) const {
    return i < 32 ? ((cfg.inflated_mask_lo >> i) & 1u) : ((cfg.inflated_mask_hi >> (i - 32)) & 1u);
  }
  bool has_skip(int i) const { return i > NL / 2; }   // temporal_denoiser.py:92
};

namespace {

void graph_drop(am_model* h) {
  if (h->gc.exec) (void)hipGraphExecDestroy(h->gc.exec);
  if (h->gc.graph) (void)hipGraphDestroy(h->gc.graph);
  h->gc.exec = nullptr; h->gc.graph = nullptr;
}

// dst_dev <- host bytes, asynchronously on `st`, safe for host memory that dies when the calling entry point returns
int stage_h2d(am_model* m, void* dst_dev, const void* src_host, size_t bytes, hipStream_t st) {
  am_model::HostStage& s = m->hstage[m->hstage_next++ % 8];
  if (s.used) AM_HIP(hipEventSynchronize(s.ev));          // the copy queued from this slot 8 uploads ago has executed
  if (s.cap < bytes) {
    if (s.pinned) AM_HIP(hipHostFree(s.pinned));
    s.pinned = nullptr;
    s.cap = bytes < 4096 ? 4096 : bytes;
    AM_HIP(hipHostMalloc(&s.pinned, s.cap, hipHostMallocDefault));
  }
  if (!s.ev) AM_HIP(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
  memcpy(s.pinned, src_host, bytes);
  AM_HIP(hipMemcpyAsync(dst_dev, s.pinned, bytes, hipMemcpyHostToDevice, st));
  AM_HIP(hipEventRecord(s.ev, st));
  s.used = true;
  return AM_OK;
}

int dev_alloc(am_model* m, void** p, size_t bytes, bool zero = true) {
  AM_HIP(hipMalloc(p, bytes ? bytes : 16));
  m->allocs.push_back(*p);
  if (zero) AM_HIP(hipMemset(*p, 0, bytes ? bytes : 16));
  return AM_OK;
}
template <class T>
int dev_alloc_t(am_model* m, T** p, size_t elems, bool zero = true) {
  return dev_alloc(m, reinterpret_cast<void**>(p), elems * sizeof(T), zero);
}

// ---- the weight table: every reference state-dict key, once.  Used by am_create / am_load_weight only. ----------
enum WKind { W_MAT, W_BIAS, W_NORM };      // bf16 matrix | fp32 vector rounded through bf16 (autocast casts the bias with the weight) | fp32 vector
enum WScope { S_TOP, S_LAYER, S_SKIP };    // the key as it stands | "blocks.<i>." + key for every layer | for the layers with a skip only
struct WDef {
  const char* key;
  WKind kind;
  WScope scope;
  void** (*dst)(am_model& m, am_layer* l);                    // where the device pointer lives
  size_t (*numel)(size_t C, size_t F, size_t Dc, size_t Din); // elements of the key
  int slot = 0, nslots = 1;                                   // a destination that concatenates several keys: this key's place in it
};
#define TOP(f) S_TOP, [](am_model& m, am_layer*) -> void** { return reinterpret_cast<void**>(&m.f); }
#define LAYER(f) S_LAYER, [](am_model&, am_layer* l) -> void** { return reinterpret_cast<void**>(&l->f); }
#define SKIP(f) S_SKIP, [](am_model&, am_layer* l) -> void** { return reinterpret_cast<void**>(&l->f); }
#define N_(expr) [](size_t C, size_t F, size_t Dc, size_t Din) -> size_t { return expr; }
const WDef kWeights[] = {
    {"time_proj.linear_1.weight", W_MAT, TOP(w_t1), N_(4 * C * C)},
    {"time_proj.linear_1.bias", W_BIAS, TOP(b_t1), N_(4 * C)},
    {"time_proj.linear_2.weight", W_MAT, TOP(w_t2), N_(4 * C * C)},
    {"time_proj.linear_2.bias", W_BIAS, TOP(b_t2), N_(C)},
    {"proj_in.weight", W_MAT, TOP(w_in), N_(C * Din)},
    {"proj_in.bias", W_BIAS, TOP(b_in), N_(C)},
    {"proj_out.weight", W_MAT, TOP(out.w), N_(Din * C)},
    {"proj_out.bias", W_BIAS, TOP(out.bias), N_(Din)},
    {"norm_out.weight", W_NORM, TOP(out.ln_w), N_(C)},
    {"norm_out.bias", W_NORM, TOP(out.ln_b), N_(C)},
    // attention_processor.py:106-110: head h reads columns [384h, 384h+384) of cat(q,k,v) => the fused weight is the plain
    // row-concatenation [Wq; Wk; Wv]
    {"s_attn.to_q.weight", W_MAT, LAYER(qkv.w), N_(C * C), 0, 3},
    {"s_attn.to_k.weight", W_MAT, LAYER(qkv.w), N_(C * C), 1, 3},
    {"s_attn.to_v.weight", W_MAT, LAYER(qkv.w), N_(C * C), 2, 3},
    {"s_attn.to_out.0.weight", W_MAT, LAYER(w_so), N_(C * C)},
    {"s_attn.to_out.0.bias", W_BIAS, LAYER(b_so), N_(C)},
    {"x_attn.to_q.weight", W_MAT, LAYER(xq.w), N_(C * C)},
    {"x_attn.to_k.weight", W_MAT, LAYER(w_xkv), N_(C * Dc), 0, 2},          // :111-115 cat(k, v)
    {"x_attn.to_v.weight", W_MAT, LAYER(w_xkv), N_(C * Dc), 1, 2},
    {"x_attn.to_out.0.weight", W_MAT, LAYER(w_xo), N_(C * C)},
    {"x_attn.to_out.0.bias", W_BIAS, LAYER(b_xo), N_(C)},
    {"ff.net.0.proj.weight", W_MAT, LAYER(ff1.w), N_(F * C)},
    {"ff.net.0.proj.bias", W_BIAS, LAYER(ff1.bias), N_(F)},
    {"ff.net.2.weight", W_MAT, LAYER(w_ff2), N_(C * F)},
    {"ff.net.2.bias", W_BIAS, LAYER(b_ff2), N_(C)},
    {"norm_s_attn.weight", W_NORM, LAYER(qkv.ln_w), N_(C)},
    {"norm_s_attn.bias", W_NORM, LAYER(qkv.ln_b), N_(C)},
    {"norm_x_attn.weight", W_NORM, LAYER(xq.ln_w), N_(C)},
    {"norm_x_attn.bias", W_NORM, LAYER(xq.ln_b), N_(C)},
    {"norm_ff.weight", W_NORM, LAYER(ff1.ln_w), N_(C)},
    {"norm_ff.bias", W_NORM, LAYER(ff1.ln_b), N_(C)},
    {"s_attn.norm_q.weight", W_NORM, LAYER(s_nq), N_(HD)},
    {"s_attn.norm_k.weight", W_NORM, LAYER(s_nk), N_(HD)},
    {"x_attn.norm_q.weight", W_NORM, LAYER(x_nq), N_(HD)},
    {"x_attn.norm_k.weight", W_NORM, LAYER(x_nk), N_(HD)},
    {"linear_skip.weight", W_MAT, SKIP(w_skip), N_(2 * C * C)},
    {"linear_skip.bias", W_BIAS, SKIP(b_skip), N_(C)},
    {"norm_skip.weight", W_NORM, SKIP(ln_k_w), N_(C)},
    {"norm_skip.bias", W_NORM, SKIP(ln_k_b), N_(C)},
};
#undef TOP
#undef LAYER
#undef SKIP
#undef N_
constexpr size_t NW = sizeof(kWeights) / sizeof(kWeights[0]);
inline size_t w_numel(const am_model* m, const WDef& w) { return w.numel(m->C, m->F, m->Dc, m->Din); }
inline bool w_exists(const am_model* m, const WDef& w, int layer) { return w.scope != S_SKIP || m->has_skip(layer); }

// The model's own keys (layer < 0) or those of one layer, in table order: one allocation per destination (slot count x element
// count) for every key the configuration has; counts those keys.
int alloc_weights(am_model* m, int layer) {
  for (const WDef& w : kWeights) {
    if ((w.scope == S_TOP) != (layer < 0) || !w_exists(m, w, layer)) continue;
    ++m->n_expected;
    if (w.slot == 0)
      AM_TRY(dev_alloc(m, w.dst(*m, layer < 0 ? nullptr : &m->layers[layer]),
                       w.nslots * w_numel(m, w) * (w.kind == W_MAT ? sizeof(bf16_t) : sizeof(float))));
  }
  return AM_OK;
}
// the products of am_ln_fold_weight for a linear of N outputs
int alloc_folded(am_model* m, am_folded& f, int N) {
  f.N = N;
  AM_TRY(dev_alloc_t(m, &f.wf, (size_t)N * m->C));
  AM_TRY(dev_alloc_t(m, &f.cs, (size_t)N));
  return dev_alloc_t(m, &f.d, (size_t)N);
}

struct WSlot { void* dst; WKind kind; size_t numel; size_t dst_off; size_t id; };
// state-dict key -> its destination in our fused layout; false for a key the table (or this configuration) does not have
bool resolve(am_model* m, const char* name, WSlot* s) {
  long li = -1;
  if (strncmp(name, "blocks.", 7) == 0) {
    char* end = nullptr;
    li = strtol(name + 7, &end, 10);
    if (end == name + 7 || *end != '.' || li < 0 || li >= m->NL) return false;
    name = end + 1;
  }
  for (size_t k = 0; k < NW; ++k) {
    const WDef& w = kWeights[k];
    if ((w.scope == S_TOP) != (li < 0) || strcmp(name, w.key) != 0) continue;
    if (!w_exists(m, w, (int)li)) return false;
    const size_t n = w_numel(m, w);
    *s = {*w.dst(*m, li < 0 ? nullptr : &m->layers[li]), w.kind, n, w.slot * n, (size_t)(li + 1) * NW + k};
    return true;
  }
  return false;
}

// C [M][N] = A [M][K] W [N][K]^T + bias, every operand dense; the setters add what a call site needs beyond that (am_gemm_args)
struct Gemm : am_gemm_args {
  Gemm() : am_gemm_args{} {}
  Gemm(const bf16_t* A, const bf16_t* Wp, const float* b, bf16_t* Cp, int ldc_, int64_t M_, int N_, int K_) : am_gemm_args{} {
    A1 = A; lda1 = K1 = ldw = K = K_; W = Wp; bias = b; C = Cp; ldc = ldc_; M = (int)M_; N = N_;
  }
  Gemm& gelu() { act = AM_GEMM_ACT_GELU; return *this; }
  Gemm& add(const bf16_t* res) { residual = res; return *this; }
  Gemm& split_a(const bf16_t* A2_, int K1_) { A2 = A2_; lda1 = K1 = K1_; lda2 = K - K1_; return *this; }   // A = [A1 | A2] by columns
  Gemm& a_rows(int G, int gs, int off) { a_G = G; a_gs = gs; a_off = off; return *this; }                  // row maps: am_gemm_args
  Gemm& c_rows(int G, int gs, int off) { c_G = G; c_gs = gs; c_off = off; return *this; }
  int run(hipStream_t st) const { return am_gemm_bf16(this, st); }
};

template <class Fn>
int for_each_folded(am_model* m, Fn fn) {
  for (am_layer& l : m->layers)
    for (am_folded* f : {&l.qkv, &l.xq, &l.ff1}) AM_TRY(fn(*f));
  return fn(m->out);
}

int prepare_folds(am_model* m, hipStream_t st) {
  {   // the synchronisation below is illegal inside a stream capture (it would invalidate it): a caller that captures the split API
      // must run one eager forward after am_load_weights first (am_denoise_forward_graph does) - say so instead
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
      AM_FAIL(AM_ERR_STATE, "%s", "the folded LayerNorm weights are built (and synchronised) by the first forward after am_load_weights: "
                                  "run one forward eagerly before capturing this stream");
    (void)hipGetLastError();
  }
  AM_TRY(for_each_folded(m, [&](am_folded& f) { return am_ln_fold_weight(f.w, f.ln_w, f.ln_b, f.bias, f.wf, f.cs, f.d, f.N, m->C, st); }));
  // once per weight load, never inside a capture: the folded weights are read by every later forward on WHATEVER stream it is
  // launched on (an eager forward on another torch stream, the graph stream after an eager call) - make them visible to all of
  // them before the flag says so (they used to be ordered only with the stream of the first forward)
  AM_HIP(hipStreamSynchronize(st));
  m->folds_ready = true;
  return AM_OK;
}

// *g = the linear `f` of LayerNorm(x) into out [rows][f.N], x = `rows` rows of the residual stream whose statistics are at `stats`.
// Folded: the un-normalised rows, their statistics and W (.) gamma.  ln_fold off: the LayerNorm kernel into h->z (trace point
// `stage`) and the plain linear.  The call site adds what differs (activation, row map, fused head split) and launches.
int ln_linear(am_model* h, const am_folded& f, const bf16_t* x, int64_t rows, const float* stats, bf16_t* out, am_trace_stage stage,
              int layer, hipStream_t st, Gemm* g) {
  if (h->ln_fold) {
    *g = Gemm(x, f.wf, f.d, out, f.N, rows, f.N, h->C);
    g->ln_stats = stats; g->ln_colsum = f.cs;
    return AM_OK;
  }
  AM_TRY(am_layernorm_bf16(x, h->z, f.ln_w, f.ln_b, rows, h->C, LN_EPS, st));
  TR(stage, layer, h->z, (size_t)rows * h->C * 2);
  *g = Gemm(h->z, f.w, f.bias, out, f.N, rows, f.N, h->C);
  return AM_OK;
}

// rows [r0, r0 + nr) of dst = A [nr][K] W^T + bias + the same rows of res (res, dst: residual-stream buffers, C columns).  With
// `want` (the next reader of these rows is a folded LayerNorm) the store loop leaves the slices of their statistics in ln_part, merged
// into ln_stats behind it.  ACTIONMESH_AMD_LN_STATS=recompute reads the rows back instead - same bits by construction (canonical
// statistics, am_common.h), which tests/test_denoiser_gpu.py asserts on whole forwards.
int residual_linear(am_model* h, const bf16_t* A, const bf16_t* W, const float* bias, int K, const bf16_t* res, bf16_t* dst, int64_t r0,
                    int64_t nr, bool want, hipStream_t st) {
  const int C = h->C, np = ceil_div(C, 256);
  const size_t off = (size_t)r0 * C;
  float *part = h->ln_part + 2 * r0 * np, *stats = h->ln_stats + 2 * r0;
  Gemm g(A, W, bias, dst + off, C, nr, C, K);
  g.add(res + off);
  if (h->ln_fold && want) g.ln_part = part;
  AM_TRY(g.run(st));
  if (!(h->ln_fold && want)) return AM_OK;
  if (h->ln_recompute) return am_row_stats_bf16(dst + off, stats, nr, C, LN_EPS, st);
  return am_row_stats_finalize(part, np, C, stats, nr, LN_EPS, st);
}

// The two attention geometries: `nseq` sequences of `sq` queries (Q in h->Qb, O to h->ao) against `nchunks` chunks of `sk` keys each.
am_attn_args attn_args(am_model* h, const bf16_t* K, const bf16_t* Vt, int nseq, int sq, int sk, int nchunks, size_t chunk_stride) {
  am_attn_args at = {};
  at.Q = h->Qb; at.K = K; at.Vt = Vt; at.O = h->ao;
  at.heads = h->H; at.ldo = h->C; at.scale = SOFTMAX_SCALE; at.defer_log2 = h->cfg.attn_defer_log2;
  at.nseq = nseq; at.sq = sq; at.sq_pad = pad_to(sq, 256);
  at.sk = sk; at.sk_pad = pad_to(sk, 64);
  at.nchunks = nchunks; at.chunk_stride = (int64_t)chunk_stride;
  return at;
}
// inflated self-attention: one sequence of T * L tokens per batch row, keys in P rank chunks (one-pass and two-pass form alike)
am_attn_args self_attn_args(am_model* h) { return attn_args(h, h->Kg, h->Vtg, h->B, h->T * h->L, h->T * h->L, h->P, h->chunk_stride); }
// per-frame self-attention and cross-attention: every frame's L queries against one chunk of its own `sk` keys
am_attn_args frame_attn_args(am_model* h, const bf16_t* K, const bf16_t* Vt, int nseq, int sk) { return attn_args(h, K, Vt, nseq, h->L, sk, 1, 0); }
// The one attention launch.  The inflated layers of an fp8 handle read the quantised operands (never a silent bf16 pass there);
// am_attention_counters counts an inflated layer once: at its one-pass launch or at the first of its two passes.
int attend(am_model* h, am_attn_args at, bool inflated, hipStream_t st) {
  const bool counted = inflated && at.state_mode != 2 && at.rows != 2;
  if (inflated && h->cfg.attn_fp8) {
    at.chunk_stride = (int64_t)h->chunk_stride8;
    if (h->cfg.attn_fp8 == 2) at.defer_log2 = AM_ATTN_FP8_FAST;
    AM_TRY(am_attention_fp8(&at, h->Q8, h->K8, h->Vt8, st));
    h->n_attn_fp8 += counted;
  } else {
    AM_TRY(am_attention_bf16(&at, st));
    h->n_attn_bf16 += counted;
  }
  return AM_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
extern "C" int am_create(const am_config* cfg, am_handle* out) {
  AM_CHECK(cfg && out, "am_create: null argument");
  AM_CHECK(cfg->num_heads > 0 && cfg->width == cfg->num_heads * HD, "am_create: width=%d must equal heads=%d * 128",
           cfg->width, cfg->num_heads);
  AM_CHECK(cfg->num_layers > 0 && cfg->num_layers <= 64, "am_create: num_layers=%d", cfg->num_layers);
  AM_CHECK(cfg->in_channels % 64 == 0 && cfg->in_channels > 0, "am_create: in_channels=%d must be a multiple of 64", cfg->in_channels);
  AM_CHECK(cfg->cross_dim % 64 == 0 && cfg->cross_dim > 0, "am_create: cross_dim=%d must be a multiple of 64", cfg->cross_dim);
  AM_CHECK(cfg->ff_inner % 64 == 0 && cfg->ff_inner > 0, "am_create: ff_inner=%d must be a multiple of 64", cfg->ff_inner);
  AM_CHECK(cfg->max_batch > 0 && cfg->max_frames_local > 0 && cfg->max_tokens > 0 && cfg->max_ctx_tokens > 0,
           "am_create: workspace bounds must be positive");
  AM_CHECK(cfg->world_size >= 1 && cfg->rank >= 0 && cfg->rank < cfg->world_size, "am_create: rank %d / world %d",
           cfg->rank, cfg->world_size);
  AM_CHECK(cfg->attn_defer_log2 == AM_ATTN_REBASE_ALWAYS || cfg->attn_defer_log2 == AM_ATTN_REBASE_DEFERRED, "am_create: attn_defer_log2 must be 0 or 8");
  AM_CHECK(cfg->attn_fp8 >= 0 && cfg->attn_fp8 <= 2, "am_create: attn_fp8 must be 0 (bf16), 1 (fp8) or 2 (fp8, exponent-field probabilities)");
  int ndev = 0;
  AM_HIP(hipGetDeviceCount(&ndev));
  AM_CHECK(ndev > 0, "am_create: no HIP device visible (this library has no CPU path)");

  am_model* m = new am_model();
  m->cfg = *cfg;
  m->C = cfg->width; m->H = cfg->num_heads; m->F = cfg->ff_inner; m->Dc = cfg->cross_dim;
  m->Din = cfg->in_channels; m->NL = cfg->num_layers; m->P = cfg->world_size; m->rank = cfg->rank;
  m->layers.resize(m->NL);
  m->loaded.assign((size_t)(m->NL + 1) * NW, 0);
  const size_t C = m->C, F = m->F, Dc = m->Dc, Din = m->Din;
  int st = AM_OK;
#define A_(call) do { if (st == AM_OK) st = (call); } while (0)
  A_(alloc_weights(m, -1)); A_(alloc_folded(m, m->out, m->Din));

  // workspace bounds
  m->maxB = cfg->max_batch; m->maxT = cfg->max_frames_local; m->maxN = cfg->max_tokens; m->maxS = cfg->max_ctx_tokens;
  m->maxL = m->maxN + 1;
  m->maxR = (int64_t)m->maxB * m->maxT * m->maxL;
  const int64_t BT = (int64_t)m->maxB * m->maxT;
  const int Spad = pad_to(m->maxS, 64);
  for (int i = 0; i < m->NL && st == AM_OK; ++i) {
    am_layer& l = m->layers[i];
    A_(alloc_weights(m, i));
    A_(alloc_folded(m, l.qkv, 3 * m->C)); A_(alloc_folded(m, l.xq, m->C)); A_(alloc_folded(m, l.ff1, m->F));
    A_(dev_alloc_t(m, &l.kx, (size_t)BT * m->H * Spad * HD));
    A_(dev_alloc_t(m, &l.vtx, (size_t)BT * m->H * HD * Spad));
  }
  const size_t R = (size_t)m->maxR;
  A_(dev_alloc_t(m, &m->hwork, R * C)); A_(dev_alloc_t(m, &m->z, R * C)); A_(dev_alloc_t(m, &m->ao, R * C));
  A_(dev_alloc_t(m, &m->qkv, R * 3 * C)); A_(dev_alloc_t(m, &m->ffh, R * F));
  m->skip.resize(m->NL / 2, nullptr);
  for (int i = 0; i < m->NL / 2; ++i) A_(dev_alloc_t(m, &m->skip[i], R * C));
  {
    const size_t q_inf = (size_t)m->maxB * m->H * pad_to((int64_t)m->maxT * m->maxL, 256) * HD;
    const size_t q_frm = (size_t)BT * m->H * pad_to(m->maxL, 256) * HD;
    A_(dev_alloc_t(m, &m->Qb, q_inf > q_frm ? q_inf : q_frm));
    const size_t k_inf = (size_t)m->maxB * m->H * pad_to((int64_t)m->maxT * m->maxL, 64) * HD;
    const size_t k_frm = (size_t)BT * m->H * pad_to(m->maxL, 64) * HD;
    m->chunk_elems = k_inf > k_frm ? k_inf : k_frm;
    m->chunk_stride = m->chunk_elems;
  }
  A_(dev_alloc_t(m, &m->xb, (size_t)BT * m->maxN * Din));
  A_(dev_alloc_t(m, &m->te0, (size_t)BT * C)); A_(dev_alloc_t(m, &m->te1, (size_t)BT * 4 * C));
  A_(dev_alloc_t(m, &m->tdev, (size_t)BT));
  A_(dev_alloc_t(m, &m->ctxb, (size_t)BT * m->maxS * Dc)); A_(dev_alloc_t(m, &m->kvtmp, (size_t)BT * m->maxS * 2 * C));
  A_(dev_alloc_t(m, &m->rope_cos, (size_t)BT * 64)); A_(dev_alloc_t(m, &m->rope_sin, (size_t)BT * 64));
  A_(dev_alloc_t(m, &m->ln_stats, R * 2)); A_(dev_alloc_t(m, &m->ln_part, R * 2 * (size_t)ceil_div((int)C, 256)));
  {
    const char* e = getenv("ACTIONMESH_AMD_LN_FOLD");       // 0: the round-3 sequence (LayerNorm kernel + plain linear), for A/B
    m->ln_fold = !(e && e[0] == '0');
    const char* r = getenv("ACTIONMESH_AMD_LN_STATS");
    m->ln_recompute = r && strcmp(r, "recompute") == 0;
  }
#undef A_
  if (st != AM_OK) {
    am_destroy(m);
    return st;
  }
  *out = m;
  return AM_OK;
}

extern "C" int am_destroy(am_handle h) {
  if (!h) return AM_OK;
  for (void* p : h->allocs) (void)hipFree(p);
  if (h->stage_f32) (void)hipFree(h->stage_f32);
  graph_drop(h);
  for (auto& s : h->hstage) {
    if (s.used) (void)hipEventSynchronize(s.ev);
    if (s.ev) (void)hipEventDestroy(s.ev);
    if (s.pinned) (void)hipHostFree(s.pinned);
  }
  delete h;
  return AM_OK;
}

extern "C" int am_load_weight(am_handle h, const char* name, const float* host, size_t numel) {
  AM_CHECK(h && name && host, "am_load_weight: null argument");
  WSlot s;
  if (!resolve(h, name, &s)) AM_FAIL(AM_ERR_NOTFOUND, "am_load_weight: unknown state-dict key '%s'", name);
  AM_CHECK(numel == s.numel, "am_load_weight: '%s' has %zu elements, expected %zu", name, numel, s.numel);
  if (s.kind == W_MAT) {
    if (h->stage_elems < numel) {
      if (h->stage_f32) AM_HIP(hipFree(h->stage_f32));
      h->stage_f32 = nullptr; h->stage_elems = 0;
      AM_HIP(hipMalloc(reinterpret_cast<void**>(&h->stage_f32), numel * sizeof(float)));
      h->stage_elems = numel;
    }
    AM_HIP(hipMemcpy(h->stage_f32, host, numel * sizeof(float), hipMemcpyHostToDevice));
    AM_TRY(am_f32_to_bf16(h->stage_f32, reinterpret_cast<bf16_t*>(s.dst) + s.dst_off, numel, nullptr));
    AM_HIP(hipStreamSynchronize(nullptr));
  } else {
    std::vector<float> tmp(host, host + numel);
    if (s.kind == W_BIAS)   // autocast casts the bias to bf16 with the weight
      for (auto& v : tmp) v = bf2f(f2bf(v));
    AM_HIP(hipMemcpy(s.dst, tmp.data(), numel * sizeof(float), hipMemcpyHostToDevice));
  }
  h->loaded[s.id] = 1;
  h->folds_ready = false;         // the folded linears (am_folded.wf, cs, d) are rebuilt by the next forward's entry point, never inside a capture
  return AM_OK;
}

extern "C" int am_weights_missing(am_handle h) {
  if (!h) return -1;
  int missing = h->n_expected;
  for (uint8_t done : h->loaded) missing -= done;
  return missing;
}

extern "C" int am_kv_chunk_elems(am_handle h, size_t* elems) {
  AM_CHECK(h && elems, "am_kv_chunk_elems: null argument");
  *elems = h->chunk_elems;
  return AM_OK;
}

extern "C" int am_bind_kv_buffers(am_handle h, uint16_t* k_dev, uint16_t* vt_dev, size_t chunk_stride_elems) {
  AM_CHECK(h && k_dev && vt_dev, "am_bind_kv_buffers: null argument");
  if (h->cfg.attn_fp8 && h->P > 1)
    AM_FAIL(AM_ERR_STATE, "am_bind_kv_buffers: an fp8 handle exchanges the QUANTISED shards - bind them with am_bind_kv8_buffers");
  AM_CHECK(((uintptr_t)k_dev | (uintptr_t)vt_dev) % 16 == 0 && chunk_stride_elems % 8 == 0, "am_bind_kv_buffers: misaligned");
  AM_CHECK(chunk_stride_elems == 0 || chunk_stride_elems >= h->chunk_elems, "am_bind_kv_buffers: chunk stride %zu < chunk size %zu",
           chunk_stride_elems, h->chunk_elems);
  h->Kg = k_dev; h->Vtg = vt_dev; h->kv_external = true;
  ++h->ctx_gen;
  h->chunk_stride = chunk_stride_elems ? chunk_stride_elems : h->chunk_elems;
  return AM_OK;
}

extern "C" int am_bind_kv8_buffers(am_handle h, uint8_t* k8_dev, uint8_t* vt8_dev, size_t chunk_stride_bytes) {
  AM_CHECK(h && k8_dev && vt8_dev, "am_bind_kv8_buffers: null argument");
  if (!h->cfg.attn_fp8) AM_FAIL(AM_ERR_STATE, "am_bind_kv8_buffers: the handle was not created with attn_fp8");
  AM_CHECK(((uintptr_t)k8_dev | (uintptr_t)vt8_dev) % 16 == 0 && chunk_stride_bytes % 16 == 0, "am_bind_kv8_buffers: misaligned");
  AM_CHECK(chunk_stride_bytes == 0 || chunk_stride_bytes >= h->chunk_elems, "am_bind_kv8_buffers: chunk stride %zu < chunk size %zu",
           chunk_stride_bytes, h->chunk_elems);
  if (h->K8 && !h->kv8_external) AM_FAIL(AM_ERR_STATE, "am_bind_kv8_buffers: bind before the first forward");
  h->K8 = k8_dev; h->Vt8 = vt8_dev; h->kv8_external = true;
  h->chunk_stride8 = chunk_stride_bytes ? chunk_stride_bytes : h->chunk_elems;
  ++h->ctx_gen;
  return AM_OK;
}

static int ensure_kv(am_model* m) {
  const bool fp8_sharded = m->cfg.attn_fp8 && m->P > 1;
  if (!m->Kg) {          // fp8 + sharding: the bf16 K / V^T are a private staging copy of the LOCAL shard only (the fp8 shards travel)
    const size_t chunks = fp8_sharded ? 1 : (size_t)m->P;
    AM_TRY(dev_alloc_t(m, &m->Kg, m->chunk_elems * chunks));
    AM_TRY(dev_alloc_t(m, &m->Vtg, m->chunk_elems * chunks));
  }
  if (m->cfg.attn_fp8) {
    if (!m->Q8) {
      const size_t q_inf = (size_t)m->maxB * m->H * pad_to((int64_t)m->maxT * m->maxL, 256) * HD;
      AM_TRY(dev_alloc_t(m, &m->Q8, q_inf));
    }
    if (!m->K8) {
      if (fp8_sharded) AM_FAIL(AM_ERR_STATE, "fp8 attention with world_size=%d: bind the fp8 gather buffers first (am_bind_kv8_buffers)", m->P);
      AM_TRY(dev_alloc_t(m, &m->K8, m->chunk_elems));
      AM_TRY(dev_alloc_t(m, &m->Vt8, m->chunk_elems));
      m->chunk_stride8 = m->chunk_elems;
    }
  }
  return AM_OK;
}

extern "C" int am_set_context(am_handle h, const float* ctx_dev, int B, int T, int S, const float* cos_host,
                              const float* sin_host, void* stream) {
  AM_CHECK(h && ctx_dev && cos_host && sin_host, "am_set_context: null argument");
  if (am_weights_missing(h) != 0) AM_FAIL(AM_ERR_STATE, "am_set_context: %d weights not loaded", am_weights_missing(h));
  AM_CHECK(B > 0 && B <= h->maxB && T > 0 && T <= h->maxT && S > 0 && S <= h->maxS,
           "am_set_context: (B=%d,T=%d,S=%d) exceeds workspace (%d,%d,%d)", B, T, S, h->maxB, h->maxT, h->maxS);
  hipStream_t st = (hipStream_t)stream;
  const int64_t BT = (int64_t)B * T;
  ++h->ctx_gen;
  AM_TRY(stage_h2d(h, h->rope_cos, cos_host, BT * 64 * sizeof(float), st));
  AM_TRY(stage_h2d(h, h->rope_sin, sin_host, BT * 64 * sizeof(float), st));
  AM_TRY(am_f32_to_bf16(ctx_dev, h->ctxb, (size_t)BT * S * h->Dc, st));
  const int Spad = pad_to(S, 64);
  for (int i = 0; i < h->NL; ++i) {
    am_layer& l = h->layers[i];
    AM_TRY(Gemm(h->ctxb, l.w_xkv, nullptr, h->kvtmp, 2 * h->C, BT * S, 2 * h->C, h->Dc).run(st));
    am_headpost_args hp = {};
    hp.X = h->kvtmp; hp.ldx = 2 * h->C; hp.rows = BT * S; hp.seq_len = S; hp.rows_per_frame = S;
    hp.heads = h->H; hp.nparts = 2; hp.kinds[0] = 1; hp.kinds[1] = 2;
    hp.w_q = nullptr; hp.w_k = l.x_nk; hp.eps = QK_EPS;
    hp.out_k = l.kx; hp.out_vt = l.vtx; hp.sk_pad = Spad;
    AM_TRY(am_head_post(&hp, st));
  }
  h->ctx_set = true; h->ctxB = B; h->ctxT = T; h->ctxS = S;
  h->ctx_zero.assign((size_t)B, 0);
  h->shared_prefix = false;
  return AM_OK;
}

extern "C" int am_set_branch_hints(am_handle h, const uint8_t* ctx_is_zero_host, int shared_prefix) {
  AM_CHECK(h, "am_set_branch_hints: null handle");
  if (!h->ctx_set) AM_FAIL(AM_ERR_STATE, "am_set_branch_hints: am_set_context has not been called");
  h->ctx_zero.assign((size_t)h->ctxB, 0);
  if (ctx_is_zero_host)
    for (int b = 0; b < h->ctxB; ++b) h->ctx_zero[b] = ctx_is_zero_host[b] ? 1 : 0;
  h->shared_prefix = shared_prefix != 0 && h->P == 1 && h->ctxB > 1;
  ++h->ctx_gen;
  return AM_OK;
}

static int forward_check(am_model* h, const float* x_dev, const float* t_bt_host, int B, int T, int N) {
  AM_CHECK(h && x_dev && t_bt_host, "am_forward_begin: null argument");
  if (!h->ctx_set) AM_FAIL(AM_ERR_STATE, "am_forward_begin: am_set_context has not been called");
  AM_CHECK(B == h->ctxB && T == h->ctxT, "am_forward_begin: (B=%d,T=%d) differs from the bound context (%d,%d)", B, T, h->ctxB, h->ctxT);
  AM_CHECK(N > 0 && N <= h->maxN, "am_forward_begin: N=%d exceeds workspace %d", N, h->maxN);
  return AM_OK;
}
// everything of am_forward_begin behind the upload of the per-frame times (h->tdev): pure device work, capturable
static int forward_begin_body(am_model* h, const float* x_dev, int B, int T, int N, hipStream_t st);

extern "C" int am_forward_begin(am_handle h, const float* x_dev, const float* t_bt_host, int B, int T, int N, void* stream) {
  AM_TRY(forward_check(h, x_dev, t_bt_host, B, T, N));
  AM_TRY(ensure_kv(h));
  hipStream_t st = (hipStream_t)stream;
  if (h->ln_fold && !h->folds_ready) AM_TRY(prepare_folds(h, st));     // weights were (re)loaded since the last forward
  AM_TRY(stage_h2d(h, h->tdev, t_bt_host, (size_t)B * T * sizeof(float), st));
  return forward_begin_body(h, x_dev, B, T, N, st);
}

static int forward_begin_body(am_model* h, const float* x_dev, int B, int T, int N, hipStream_t st) {
  const int C = h->C, Din = h->Din;
  h->B = B; h->T = T; h->N = N; h->L = N + 1; h->R = (int64_t)B * T * h->L;
  const int64_t BT = (int64_t)B * T;
  // proj_in (temporal_denoiser.py:205-206) written behind each frame's time token (:217)
  AM_TRY(am_f32_to_bf16(x_dev, h->xb, (size_t)BT * N * Din, st));
  AM_TRY(Gemm(h->xb, h->w_in, h->b_in, h->hwork, C, BT * N, C, Din).c_rows(N, h->L, 1).run(st));
  // time token (:213-217): sinusoid -> Linear -> GELU -> Linear -> row 0 of each frame
  AM_TRY(am_timestep_sinusoid(h->tdev, h->te0, (int)BT, C, st));
  AM_TRY(Gemm(h->te0, h->w_t1, h->b_t1, h->te1, 4 * C, BT, 4 * C, C).gelu().run(st));
  AM_TRY(Gemm(h->te1, h->w_t2, h->b_t2, h->hwork, C, BT, C, 4 * C).c_rows(1, h->L, 0).run(st));
  TR(TR_PROJ_IN, 0, h->hwork, (size_t)h->R * C * 2);
  if (h->ln_fold) AM_TRY(am_row_stats_bf16(h->hwork, h->ln_stats, h->R, C, LN_EPS, st));
  h->hsrc = h->hwork;
  h->skip_top = 0;
  h->next_layer = 0;
  h->pre_done = false;
  h->in_forward = true;
  return AM_OK;
}

// A bias-free projection fused with its head split (am_gemm_headpost_bf16); trace runs keep the two launches apart so that the
// linear's output can be checksummed
static int linear_head_split(const Gemm& g, const am_headpost_args& hp, am_trace_stage stage, int layer, hipStream_t st) {
  if (!am_trace_on()) return am_gemm_headpost_bf16(&g, &hp, st);
  AM_TRY(g.run(st));
  TR(stage, layer, hp.X, (size_t)hp.rows * hp.ldx * 2);
  return am_head_post(&hp, st);
}

extern "C" int am_layer_pre_attn(am_handle h, int i, void* stream) {
  AM_CHECK(h, "am_layer_pre_attn: null handle");
  if (!h->in_forward || i != h->next_layer || h->pre_done)
    AM_FAIL(AM_ERR_STATE, "am_layer_pre_attn: layer %d out of order (next=%d)", i, h->next_layer);
  hipStream_t st = (hipStream_t)stream;
  am_layer& l = h->layers[i];
  const int C = h->C, L = h->L;
  const int64_t R = h->R;
  if (h->has_skip(i)) {   // block.py:131-133
    AM_CHECK(h->skip_top > 0, "am_layer_pre_attn: skip stack empty at layer %d", i);
    const bf16_t* sk = h->skip[--h->skip_top];
    AM_TRY(Gemm(sk, l.w_skip, l.b_skip, h->z, C, R, C, 2 * C).split_a(h->hsrc, C).run(st));
    TR(TR_SKIP_LINEAR, i, h->z, (size_t)R * C * 2);
    if (h->ln_fold) AM_TRY(am_layernorm_stats_bf16(h->z, h->hwork, l.ln_k_w, l.ln_k_b, R, C, LN_EPS, h->ln_stats, st));
    else AM_TRY(am_layernorm_bf16(h->z, h->hwork, l.ln_k_w, l.ln_k_b, R, C, LN_EPS, st));
    TR(TR_SKIP_NORM, i, h->hwork, (size_t)R * C * 2);
    h->hsrc = h->hwork;
  }
  // exact shortcut (am_set_branch_hints): until the first cross-attention every batch row is the same tensor - layer 0's
  // self-attention branch runs on row 0 only and am_layer_post_attn copies its result to the other rows
  const bool shared = i == 0 && h->shared_prefix && !h->has_skip(0);
  const int64_t Rs = shared ? R / h->B : R;
  // norm_s_attn (block.py:138) -> the q | k | v projection (:92-103) -> head split, qk-norm, RoPE into the attention operand layouts
  const bool inflated = h->inflated(i), fp8_sharded = h->cfg.attn_fp8 && h->P > 1;
  const am_attn_args at = inflated ? self_attn_args(h) : frame_attn_args(h, h->Kg, h->Vtg, h->B * h->T, L);
  Gemm gq;
  AM_TRY(ln_linear(h, l.qkv, h->hsrc, Rs, h->ln_stats, h->qkv, TR_NORM_S, i, st, &gq));
  am_headpost_args hp = {};
  hp.X = h->qkv; hp.ldx = 3 * C; hp.rows = Rs; hp.seq_len = at.sq; hp.rows_per_frame = L;
  hp.heads = h->H; hp.nparts = 3; hp.kinds[0] = 0; hp.kinds[1] = 1; hp.kinds[2] = 2;
  hp.w_q = l.s_nq; hp.w_k = l.s_nk; hp.eps = QK_EPS;
  hp.rope_cos = h->rope_cos; hp.rope_sin = h->rope_sin;
  hp.out_q = h->Qb; hp.sq_pad = at.sq_pad; hp.sk_pad = at.sk_pad;
  // an inflated layer writes this rank's chunk of the gather buffers (fp8 + sharding: Kg / Vtg hold the local shard only - ensure_kv)
  const size_t own = inflated && !fp8_sharded ? (size_t)h->rank * h->chunk_stride : 0;
  hp.out_k = h->Kg + own; hp.out_vt = h->Vtg + own;
  AM_TRY(linear_head_split(gq, hp, TR_QKV, i, st));
  TR(TR_HP_Q, i, h->Qb, (size_t)at.nseq * h->H * hp.sq_pad * HD * 2);
  TR(TR_HP_KV, i, hp.out_k, h->chunk_elems * 2);
  TR(TR_HP_KV, i, hp.out_vt, h->chunk_elems * 2);
  if (inflated && h->cfg.attn_fp8) {
    // fp8 variant: Q and THIS rank's K / V^T shard are quantised here, so that with world_size > 1 the shards that travel are the
    // fp8 ones (half the bytes on the links, and every rank quantises 1 / P of the keys instead of all of them after the gather)
    am_attn_args qa = at;
    if (shared) qa.nseq /= h->B;
    qa.K = hp.out_k; qa.Vt = hp.out_vt; qa.nchunks = 1; qa.chunk_stride = 0;
    AM_TRY(am_attention_quantize_fp8(&qa, h->Q8, h->K8 + (size_t)h->rank * h->chunk_stride8, h->Vt8 + (size_t)h->rank * h->chunk_stride8, st));
  }
  h->pre_done = true;
  return AM_OK;
}

// Multi-GPU overlap: between am_layer_pre_attn and am_layer_post_attn of an inflated layer, while the all-gather of
// the other ranks' K / V^T shards is in flight, run the self-attention of the full query blocks against the LOCAL
// shard only and park the un-normalised (O, m, l).  am_layer_post_attn then resumes over the remote shards.
// A no-op (AM_OK) when the layer / shapes do not qualify: post_attn falls back to the one-pass attention.
extern "C" int am_layer_attn_local(am_handle h, int i, void* stream) {
  AM_CHECK(h, "am_layer_attn_local: null handle");
  if (!h->in_forward || i != h->next_layer || !h->pre_done)
    AM_FAIL(AM_ERR_STATE, "am_layer_attn_local: layer %d out of order (next=%d)", i, h->next_layer);
  hipStream_t st = (hipStream_t)stream;
  h->local_done = false;
  const int tiles = (h->T * h->L + 63) / 64;
  const bool product = h->cfg.attn_defer_log2 == AM_ATTN_REBASE_ALWAYS || h->cfg.attn_defer_log2 == AM_ATTN_REBASE_DEFERRED;
  if (h->P < 2 || !h->inflated(i) || tiles < 16 || !product) return AM_OK;
  am_attn_args at = self_attn_args(h);
  if (!h->attn_state)
    AM_TRY(dev_alloc_t(h, &h->attn_state, (size_t)h->maxB * h->H * pad_to((int64_t)h->maxT * h->maxL, 256) * AM_ATTN_STATE_LD));
  at.rows = 1; at.state_mode = 1; at.state = h->attn_state;
  at.nchunks = 1; at.chunk_first = h->rank; at.chunk_total = h->P;
  AM_TRY(attend(h, at, true, st));
  TR(TR_ATTN_LOCAL_STATE, i, h->attn_state, (size_t)at.nseq * at.heads * at.sq_pad * AM_ATTN_STATE_LD * 4);
  h->local_done = true;
  return AM_OK;
}

extern "C" int am_layer_post_attn(am_handle h, int i, void* stream) {
  AM_CHECK(h, "am_layer_post_attn: null handle");
  if (!h->in_forward || i != h->next_layer || !h->pre_done)
    AM_FAIL(AM_ERR_STATE, "am_layer_post_attn: layer %d out of order (next=%d)", i, h->next_layer);
  hipStream_t st = (hipStream_t)stream;
  am_layer& l = h->layers[i];
  const int C = h->C, L = h->L, F = h->F;
  const int64_t R = h->R;
  const bool inflated = h->inflated(i);
  const bool shared = i == 0 && h->shared_prefix && !h->has_skip(0);
  const int64_t Rs = shared ? R / h->B : R;
  // ---- self-attention (attention_processor.py:133-166) ------------------------
  if (inflated && h->local_done) {
    // second pass: the full blocks resume from the saved state over the P-1 remote shards (rank+1 .. rank-1, wrapping);
    // the short last block runs one pass over all shards
    am_attn_args rest = self_attn_args(h), at = rest;
    at.rows = 1; at.state_mode = 2; at.state = h->attn_state;
    at.nchunks = h->P - 1; at.chunk_first = (h->rank + 1) % h->P; at.chunk_total = h->P;
    if (am_trace_on()) {
      // the shards the attention really reads: an fp8 handle with P > 1 gathers QUANTISED shards in K8 / Vt8 (Kg / Vtg then hold one
      // chunk only - ensure_kv - so walking P chunks of them would read out of bounds)
      const bool fp8_sharded = h->cfg.attn_fp8 && h->P > 1;
      for (int c = 0; c < h->P; ++c) {
        if (fp8_sharded) {
          TR(TR_KV_CHUNKS, i, h->K8 + (size_t)c * h->chunk_stride8, h->chunk_elems);
          TR(TR_KV_CHUNKS, i, h->Vt8 + (size_t)c * h->chunk_stride8, h->chunk_elems);
        } else {
          TR(TR_KV_CHUNKS, i, h->Kg + (size_t)c * h->chunk_stride, h->chunk_elems * 2);
          TR(TR_KV_CHUNKS, i, h->Vtg + (size_t)c * h->chunk_stride, h->chunk_elems * 2);
        }
      }
      TR(TR_Q_BEFORE_ATTN, i, h->Qb, (size_t)at.nseq * at.heads * at.sq_pad * HD * 2);
      TR(TR_STATE_BEFORE_RESUME, i, h->attn_state, (size_t)at.nseq * at.heads * at.sq_pad * AM_ATTN_STATE_LD * 4);
    }
    AM_TRY(attend(h, at, true, st));
    TR(TR_ATTN_RESUME, i, h->ao, (size_t)Rs * C * 2);
    rest.rows = 2;
    AM_TRY(attend(h, rest, true, st));
    TR(TR_ATTN_LAST_BLOCK, i, h->ao, (size_t)Rs * C * 2);
    h->local_done = false;
  } else {
    am_attn_args at = inflated ? self_attn_args(h) : frame_attn_args(h, h->Kg, h->Vtg, h->B * h->T, L);
    if (shared) at.nseq /= h->B;                           // row 0's sequences only (they come first in every layout)
    AM_TRY(attend(h, at, inflated, st));
    TR(TR_ATTN_ONE_PASS, i, h->ao, (size_t)Rs * C * 2);
  }
  // to_out + residual (block.py:137)
  AM_TRY(residual_linear(h, h->ao, l.w_so, l.b_so, C, h->hsrc, h->hwork, 0, Rs, true, st));
  TR(TR_TO_OUT, i, h->hwork, (size_t)Rs * C * 2);
  if (shared)
    for (int b = 1; b < h->B; ++b) {
      AM_HIP(hipMemcpyAsync(h->hwork + (size_t)b * Rs * C, h->hwork, (size_t)Rs * C * sizeof(bf16_t), hipMemcpyDeviceToDevice, st));
      if (h->ln_fold)
        AM_HIP(hipMemcpyAsync(h->ln_stats + (size_t)b * Rs * 2, h->ln_stats, (size_t)Rs * 2 * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
  h->hsrc = h->hwork;
  // ---- cross-attention to the frame's own context tokens (block.py:146-149) ----
  // Batch rows whose context is identically zero (am_set_branch_hints: the unconditional guidance branch) get the exact
  // result of the branch - h += to_out bias - instead of the branch; the others run it, one contiguous run of rows at a time.
  const int64_t R1 = R / h->B;                       // rows of one batch row
  for (int b0 = 0, b1; b0 < h->B; b0 = b1) {
    const bool zero = !h->ctx_zero.empty() && h->ctx_zero[b0];
    for (b1 = b0 + 1; b1 < h->B && (!h->ctx_zero.empty() && h->ctx_zero[b1]) == zero;) ++b1;
    const int64_t r0 = (int64_t)b0 * R1, nr = (int64_t)(b1 - b0) * R1;
    bf16_t* hrun = h->hwork + (size_t)r0 * C;
    if (zero) {
      if (h->ln_fold) AM_TRY(am_add_bias_rows_stats(hrun, l.b_xo, nr, C, LN_EPS, h->ln_stats + 2 * r0, st));
      else AM_TRY(am_add_bias_rows(hrun, l.b_xo, nr, C, st));
      TR(TR_X_BIAS_ONLY, i, hrun, (size_t)nr * C * 2);
      continue;
    }
    Gemm gx;                   // norm_x_attn (block.py:146) -> to_q -> head split, qk-norm
    AM_TRY(ln_linear(h, l.xq, hrun, nr, h->ln_stats + 2 * r0, h->qkv, TR_NORM_X, i, st, &gx));
    am_headpost_args hp = {};
    hp.X = h->qkv; hp.ldx = C; hp.rows = nr; hp.seq_len = L; hp.rows_per_frame = L;
    hp.heads = h->H; hp.nparts = 1; hp.kinds[0] = 0;
    hp.w_q = l.x_nq; hp.eps = QK_EPS;
    hp.out_q = h->Qb; hp.sq_pad = pad_to(L, 256);
    AM_TRY(linear_head_split(gx, hp, TR_XQ, i, st));
    TR(TR_X_HP_Q, i, h->Qb, (size_t)(b1 - b0) * h->T * h->H * hp.sq_pad * HD * 2);
    const size_t kv0 = (size_t)b0 * h->T * h->H * pad_to(h->ctxS, 64) * HD;      // the run's first frame in the K / V^T cache
    AM_TRY(attend(h, frame_attn_args(h, l.kx + kv0, l.vtx + kv0, (b1 - b0) * h->T, h->ctxS), false, st));
    TR(TR_X_ATTN, i, h->ao, (size_t)nr * C * 2);
    AM_TRY(residual_linear(h, h->ao, l.w_xo, l.b_xo, C, h->hwork, h->hwork, r0, nr, true, st));
    TR(TR_X_TO_OUT, i, hrun, (size_t)nr * C * 2);
  }
  // ---- feed-forward (block.py:152; diffusers FeedForward "gelu"): norm_ff -> ff.net.0 + GELU -> ff.net.2 + residual --------------
  Gemm g1;
  AM_TRY(ln_linear(h, l.ff1, h->hwork, R, h->ln_stats, h->ffh, TR_NORM_FF, i, st, &g1));
  AM_TRY(g1.gelu().run(st));
  TR(TR_FF1, i, h->ffh, (size_t)R * F * 2);
  bf16_t* dst = h->hwork;
  if (i < h->NL / 2) dst = h->skip[h->skip_top++];     // temporal_denoiser.py:231-232 (kept, not copied)
  // the next reader of the row statistics is the next block's norm_s_attn - unless that block starts with its skip linear + norm_skip
  // (which writes its own); behind the last block the reader is norm_out, folded into proj_out (am_forward_end)
  AM_TRY(residual_linear(h, h->ffh, l.w_ff2, l.b_ff2, F, h->hwork, dst, 0, R, i + 1 >= h->NL || !h->has_skip(i + 1), st));
  TR(TR_FF2, i, dst, (size_t)R * C * 2);
  h->hsrc = dst;
  h->next_layer = i + 1;
  h->pre_done = false;
  return AM_OK;
}

extern "C" int am_forward_end(am_handle h, uint16_t* v_out, void* stream) {
  AM_CHECK(h && v_out, "am_forward_end: null argument");
  if (!h->in_forward || h->next_layer != h->NL) AM_FAIL(AM_ERR_STATE, "am_forward_end: %d of %d layers run", h->next_layer, h->NL);
  hipStream_t st = (hipStream_t)stream;
  // norm_out -> drop the time token -> proj_out (temporal_denoiser.py:239-242).  Folded like the three LayerNorms of a block: the last
  // ff.net.2 left the row statistics of the residual stream, proj_out reads the un-normalised rows through its row map.
  Gemm g;
  AM_TRY(ln_linear(h, h->out, h->hsrc, h->R, h->ln_stats, v_out, TR_NORM_OUT, 0, st, &g));
  g.M = (int)((int64_t)h->B * h->T * h->N);
  AM_TRY(g.a_rows(h->N, h->L, 1).run(st));
  TR(TR_PROJ_OUT, 0, v_out, (size_t)h->B * h->T * h->N * h->Din * 2);
  h->in_forward = false;
  return AM_OK;
}

extern "C" int am_denoise_forward(am_handle h, const float* x_dev, const float* t_bt_host, int B, int T, int N,
                                  uint16_t* v_out, void* stream) {
  AM_CHECK(h, "am_denoise_forward: null handle");
  if (h->P != 1) AM_FAIL(AM_ERR_STATE, "am_denoise_forward: world_size=%d needs the split API with a K/V all-gather", h->P);
  AM_TRY(am_forward_begin(h, x_dev, t_bt_host, B, T, N, stream));
  for (int i = 0; i < h->NL; ++i) {
    AM_TRY(am_layer_pre_attn(h, i, stream));
    AM_TRY(am_layer_post_attn(h, i, stream));
  }
  return am_forward_end(h, v_out, stream);
}

// am_denoise_forward through a HIP graph: the ~450 launches of a forward are captured once per (operands, shape, stream, window)
// and replayed; only the upload of the per-frame diffusion times stays outside the graph.  First call with a new key: eager (it
// also performs every lazy allocation / attribute call a capture must not contain); second: capture + instantiate + launch;
// later: launch.  A capture that fails disables the graph path for the handle (eager from then on, counted in am_graph_stats).
static int forward_body(am_model* h, const float* x_dev, int B, int T, int N, uint16_t* v_out, hipStream_t st) {
  AM_TRY(forward_begin_body(h, x_dev, B, T, N, st));
  for (int i = 0; i < h->NL; ++i) {
    AM_TRY(am_layer_pre_attn(h, i, st));
    AM_TRY(am_layer_post_attn(h, i, st));
  }
  return am_forward_end(h, v_out, st);
}
extern "C" int am_denoise_forward_graph(am_handle h, const float* x_dev, const float* t_bt_host, int B, int T, int N,
                                        uint16_t* v_out, void* stream) {
  AM_CHECK(h && v_out, "am_denoise_forward_graph: null argument");
  if (h->P != 1) AM_FAIL(AM_ERR_STATE, "am_denoise_forward_graph: world_size=%d needs the split API", h->P);
  am_model::GraphCache& g = h->gc;
  hipStream_t st = (hipStream_t)stream;
  if (g.disabled || st == nullptr) {          // the legacy null stream cannot be captured
    ++g.eager;
    return am_denoise_forward(h, x_dev, t_bt_host, B, T, N, v_out, stream);
  }
  AM_TRY(forward_check(h, x_dev, t_bt_host, B, T, N));
  if (h->ln_fold && !h->folds_ready) AM_TRY(prepare_folds(h, st));     // in front of a replay or a capture, never inside one
  const bool same = g.x == x_dev && g.v == v_out && g.B == B && g.T == T && g.N == N && g.st == st && g.ctx_gen == h->ctx_gen &&
                    g.scratch_gen == g_am_scratch_generation.load();
  if (!same) {
    graph_drop(h);
    g.x = x_dev; g.v = v_out; g.B = B; g.T = T; g.N = N; g.st = st; g.ctx_gen = h->ctx_gen; g.warm = true;
    ++g.eager;
    const int rc0 = am_denoise_forward(h, x_dev, t_bt_host, B, T, N, v_out, stream);
    g.scratch_gen = g_am_scratch_generation.load();      // after the eager run: it may have grown the scratch
    return rc0;
  }
  AM_TRY(stage_h2d(h, h->tdev, t_bt_host, (size_t)B * T * sizeof(float), st));
  if (!g.exec) {
    AM_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    const int rc = forward_body(h, x_dev, B, T, N, v_out, st);
    hipGraph_t gr = nullptr;
    const hipError_t e = hipStreamEndCapture(st, &gr);
    hipError_t e2 = hipSuccess;
    if (rc == AM_OK && e == hipSuccess && gr) e2 = hipGraphInstantiate(&g.exec, gr, nullptr, nullptr, 0);
    if (rc != AM_OK || e != hipSuccess || !gr || e2 != hipSuccess || !g.exec) {
      (void)hipGetLastError();
      if (gr) (void)hipGraphDestroy(gr);
      g.exec = nullptr; g.disabled = true; h->in_forward = false;
      ++g.eager;
      return am_denoise_forward(h, x_dev, t_bt_host, B, T, N, v_out, stream);
    }
    g.graph = gr;
    ++g.captures;
  } else {
    ++g.replays;
  }
  AM_HIP(hipGraphLaunch(g.exec, st));
  return AM_OK;
}
// counts[0] = graph launches of an existing executable, [1] = captures, [2] = eager forwards (first use of a key, null stream,
// or after a failed capture), [3] = 1 when a capture has failed and the graph path is off
extern "C" int am_graph_stats(am_handle h, uint64_t* counts4) {
  AM_CHECK(h && counts4, "am_graph_stats: null argument");
  counts4[0] = h->gc.replays; counts4[1] = h->gc.captures; counts4[2] = h->gc.eager; counts4[3] = h->gc.disabled ? 1 : 0;
  return AM_OK;
}

// counts2 = {fp8, bf16} inflated self-attention launches of this handle so far (a two-pass layer counts once): what a run really
// computed in, whatever it was configured for - bench.py derives its `dtype` and `roofline.peak` from this.
extern "C" int am_attention_counters(am_handle h, uint64_t* counts2) {
  AM_CHECK(h && counts2, "am_attention_counters: null argument");
  counts2[0] = h->n_attn_fp8; counts2[1] = h->n_attn_bf16;
  return AM_OK;
}

extern "C" double am_step_flops(am_handle h, int B, int T, int N, int S) {
  if (!h) return 0.0;
  const double C = h->C, F = h->F, Dc = h->Dc, Din = h->Din;
  const double TL = (double)T * (N + 1);
  double tot = 0.0;
  for (int i = 0; i < h->NL; ++i) {
    const double attn = h->inflated(i) ? 4.0 * TL * TL * C : 4.0 * T * (double)(N + 1) * (N + 1) * C;
    double per = 6.0 * TL * C * C + attn + 2.0 * TL * C * C;
    per += 2.0 * TL * C * C + 4.0 * T * S * Dc * C + 4.0 * TL * S * C + 2.0 * TL * C * C;
    per += 4.0 * TL * C * F;
    if (h->has_skip(i)) per += 4.0 * TL * C * C;
    tot += per;
  }
  tot += 4.0 * T * N * Din * C + 16.0 * T * C * C;
  return B * tot;
}
