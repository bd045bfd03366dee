"""Kernel-level Python wrappers over the C-ABI (torch tensors in, raw pointers out).

These are thin marshalling helpers: torch provides device memory and the current
HIP stream, the arithmetic is entirely in libactionmesh_amd.so.  Used by the
parity tests and by the attention-processor seam (S3).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence, Tuple

import torch

from . import _lib as L
from .mesh_topology import MeshTopology

HEAD_DIM = 128


H16 = (torch.bfloat16, torch.float16)       # the two 16-bit storage types: each has its own build of the library (_lib.lib(kind))


def _entry(key, name: str):
    """(library, its entry point `name`).  `key` picks the build: a tensor or dtype (float16 -> libactionmesh_amd_f16.so, the same sources
    built with -DAM_F16; anything else -> libactionmesh_amd.so), a kind "bf16" / "f16" (the fp32 entry points are in both builds: the
    caller says which one runs them), or None for the entry points that have no 16-bit code (the bfloat16 build)."""
    if isinstance(key, torch.Tensor):
        key = key.dtype
    l = L.lib(key if isinstance(key, str) else "f16" if key == torch.float16 else "bf16")
    return l, getattr(l, name)


def _call(t: torch.Tensor, key, name: str, *args) -> None:
    """Call the C-ABI kernel entry point `name` (of the build `key` picks, see _entry) on the device that owns `t`: the device is made
    current for the call (the library launches on the current device) and the stream, the entry point's last argument, is torch's
    current stream OF THAT DEVICE, so a tensor on a non-current device is neither launched on device 0's stream nor unordered with the
    work that produced it.  A non-zero status raises with the am_last_error of the library that ran."""
    l, fn = _entry(key, name)
    with torch.cuda.device(t.device):
        L.check(fn(*args, torch.cuda.current_stream(t.device).cuda_stream), name, l)


def _workspace(device, query: str, *dims, at_least: int = 0) -> Tuple[Optional[torch.Tensor], int]:
    """The scratch buffer of an entry point: (uint8 tensor, the byte count to declare to the library) for the size its `query`
    function (am_*_workspace_bytes) returns for `dims`.  `at_least`: the smallest buffer allocated whatever the size - an entry point
    that refuses a null workspace gets a real pointer for a size of 0; with 0, a size of 0 allocates nothing (tensor None)."""
    need = _entry(None, query)[1](*dims)
    size = max(need, at_least)
    return (torch.empty((size,), dtype=torch.uint8, device=device) if size else None), need


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _on_device(t: torch.Tensor, dtype, name: str) -> None:
    """The check every operand passes: a device tensor of `dtype` (one dtype or a tuple of them)."""
    if not t.is_cuda:
        raise RuntimeError(f"{name}: actionmesh_amd kernels need a device tensor (no CPU path)")
    if (t.dtype not in dtype) if isinstance(dtype, tuple) else (t.dtype != dtype):
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")


def _need(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    """A contiguous device tensor of `dtype`."""
    _on_device(t, dtype, name)
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t


def _need_rows(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    """A 2-D device tensor of `dtype` with unit column stride: an operand whose leading dimension (t.stride(0)) goes to the library,
    so rows may be padded or be a column slice of a wider buffer (of a packed projection output, say).  Contiguous 2-D tensors qualify."""
    _on_device(t, dtype, name)
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: expected a 2-D tensor with unit column stride, got shape {tuple(t.shape)} strides {t.stride()}")
    return t


def _need_head_columns(who: str, name: str, t: torch.Tensor, heads: int, off: int, hs: int, head_dim: int) -> None:
    """Packed heads of the fp32 path: head h of a row of `t` is columns [off + h * hs, + head_dim); the last one ends inside the row."""
    end = off + (heads - 1) * hs + head_dim
    if heads < 1 or off < 0 or hs < 0 or end > t.shape[1]:
        raise ValueError(f"{who}: {name} has {t.shape[1]} columns, head {heads - 1} ends at {end}")


def _need_rope_tables(who: str, rope: Tuple[torch.Tensor, torch.Tensor], rows: int, rows_per_frame: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """`rope` = (cos, sin), each (frames, 64) fp32; row r takes frame r // rows_per_frame, and the rows stay inside the frames."""
    cos, sin = rope
    _need(cos, torch.float32, "rope cos"); _need(sin, torch.float32, "rope sin")
    if cos.dim() != 2 or cos.shape[1] != HEAD_DIM // 2 or sin.shape != cos.shape:
        raise ValueError(f"{who}: rope tables must be (frames, {HEAD_DIM // 2}), got {tuple(cos.shape)} / {tuple(sin.shape)}")
    if rows_per_frame < 1 or (rows - 1) // rows_per_frame >= cos.shape[0]:
        raise ValueError(f"{who}: {rows} rows of {rows_per_frame} per frame run past the {cos.shape[0]} frames of the tables")
    return cos, sin


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def _out_rows(out: Optional[torch.Tensor], rows: int, ld_out: int, dtype, device, name: str) -> torch.Tensor:
    """The (rows, ld_out) output of a kernel that writes whole rows of `ld_out` elements: a fresh tensor, or the caller's `out`."""
    if out is None:
        return torch.empty((rows, ld_out), dtype=dtype, device=device)
    _need(out, dtype, f"{name}: out")
    if tuple(out.shape) != (rows, ld_out):
        raise ValueError(f"{name}: out {tuple(out.shape)} != ({rows}, {ld_out})")
    return out


def perm16_index(n: int, device=None) -> torch.Tensor:
    """position -> key index map of the V^T layout (bit2 <-> bit3 inside each 16-group)."""
    k = torch.arange(n, device=device)
    return (k & ~0xC) | ((k & 4) << 1) | ((k & 8) >> 1)


def _fold_args(g, bias: Optional[torch.Tensor], ln: Optional[Tuple[torch.Tensor, torch.Tensor]]) -> None:
    """The bias and the folded LayerNorm (`ln` = (stats, colsum)) of a linear into its AmGemmArgs."""
    if bias is not None:
        g.bias = _need(bias, torch.float32, "bias").data_ptr()
    if ln is not None:
        g.ln_stats = _need(ln[0], torch.float32, "ln stats").data_ptr()
        g.ln_colsum = _need(ln[1], torch.float32, "ln colsum").data_ptr()


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
         residual: Optional[torch.Tensor] = None, gelu: bool = False,
         a2: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
         a_map: Tuple[int, int, int] = (0, 0, 0), c_map: Tuple[int, int, int] = (0, 0, 0),
         M: Optional[int] = None, force_small: bool = False, legacy: bool = False,
         force_big: bool = False, ablate: int = 0,
         ln: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, ln_part: Optional[torch.Tensor] = None,
         gelu_table: bool = True) -> torch.Tensor:
    """out = act(cat(a, a2) @ w.T + bias) + residual   (bf16, fp32 accumulate).

    a (Ma, K1), a2 (Ma, K2) optional, w (N, K1+K2), bias fp32 (N,), residual/out (Mc, N).
    a_map / c_map = (G, group_stride, offset) row maps (G=0: identity).
    ln = (stats (M, 2) fp32, colsum (N,) fp32): the LayerNorm of `a` folded into the linear (w, bias from ln_fold_weight; see
    am_gemm_args in include/actionmesh_amd.h).  ln_part (M, ceil(N / 256), 2) fp32: receives the per-slice (mean, M2) of the output rows."""
    _need_rows(a, H16, "a"); _need_rows(w, a.dtype, "w")
    K1 = a.shape[1]
    K = w.shape[1]
    N = w.shape[0]
    if M is None:
        M = a.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=a.dtype, device=a.device)
    _need_rows(out, a.dtype, "out")
    g = L.AmGemmArgs()
    g.A1 = a.data_ptr(); g.lda1 = a.stride(0); g.K1 = K1
    g.A2 = _p(a2); g.lda2 = a2.stride(0) if a2 is not None else 0
    if a2 is not None:
        _need_rows(a2, a.dtype, "a2")
        assert K1 + a2.shape[1] == K
    else:
        assert K1 == K
    g.W = w.data_ptr(); g.ldw = w.stride(0)
    _fold_args(g, bias, ln)
    g.residual = _p(_need_rows(residual, a.dtype, "residual")) if residual is not None else None
    g.C = out.data_ptr(); g.ldc = out.stride(0)
    g.M, g.N, g.K = M, N, K
    # beside the activation, the diagnostic and test switches of `act` (AM_GEMM_* in include/actionmesh_amd.h): the kernel choice, the
    # timing ablations and start skew of `ablate`, the arithmetic GELU epilogue
    g.act = (L.GEMM_ACT_GELU if gelu else 0) | (L.GEMM_FORCE_128 if force_small else 0) | (L.GEMM_LOCKSTEP if legacy else 0) \
        | (L.GEMM_FORCE_256 if force_big else 0) | (ablate & (L.GEMM_ABLATE_MASK | L.GEMM_SKEW_MASK)) | (0 if gelu_table else L.GEMM_NO_GELU_TABLE)
    g.a_G, g.a_gs, g.a_off = a_map
    g.c_G, g.c_gs, g.c_off = c_map
    if ln is not None:
        assert ln[0].numel() >= 2 * M and ln[1].numel() == N
    if ln_part is not None:
        _need(ln_part, torch.float32, "ln_part")
        assert ln_part.numel() >= 2 * M * ((N + 255) // 256)
        g.ln_part = ln_part.data_ptr()
    _call(a, a, "am_gemm_bf16", C.byref(g))
    return out


def row_stats(x: torch.Tensor, eps: float = 1e-5, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(mean, rstd) per row of x (rows, C): fp32 (rows, 2) - the statistics layernorm() uses, for gemm(..., ln=...)."""
    _need(x, H16, "x")
    Cdim = x.shape[-1]
    rows = x.numel() // Cdim
    if out is None:
        out = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
    _call(x, x, "am_row_stats_bf16", x.data_ptr(), _need(out, torch.float32, "out").data_ptr(), rows, Cdim, eps)
    return out


def row_stats_finalize(part: torch.Tensor, Cdim: int, eps: float = 1e-5, out: Optional[torch.Tensor] = None, kind=torch.bfloat16) -> torch.Tensor:
    """part (rows, ceil(Cdim / 256), 2) fp32 pairs (mean, M2) of 256-column slices (gemm(..., ln_part=...)) -> (rows, 2) (mean, rstd)."""
    _need(part, torch.float32, "part")
    rows, nparts = part.shape[0], part.shape[1]
    if out is None:
        out = torch.empty((rows, 2), dtype=torch.float32, device=part.device)
    _call(part, kind, "am_row_stats_finalize", part.data_ptr(), nparts, Cdim, out.data_ptr(), rows, eps)
    return out


def ln_fold_weight(w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, bias: Optional[torch.Tensor] = None,
                   out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None):
    """One-time preparation of a linear that absorbs the LayerNorm in front of it: returns (wf, colsum, d) for gemm(a, wf, bias=d,
    ln=(row_stats(a), colsum)) == gemm(layernorm(a, gamma, beta), w, bias) up to the bf16 rounding of the normalised activation."""
    _need(w, H16, "w"); _need(gamma, torch.float32, "gamma"); _need(beta, torch.float32, "beta")
    N, K = w.shape
    if out is None:
        wf = torch.empty_like(w)
        colsum = torch.empty((N,), dtype=torch.float32, device=w.device)
        d = torch.empty((N,), dtype=torch.float32, device=w.device)
    else:       # caller-owned (wf (N, K), colsum (N,), d (N,))
        wf, colsum, d = _need(out[0], w.dtype, "out wf"), _need(out[1], torch.float32, "out colsum"), _need(out[2], torch.float32, "out d")
        if tuple(wf.shape) != (N, K) or colsum.numel() != N or d.numel() != N:
            raise ValueError(f"ln_fold_weight: out shapes {tuple(wf.shape)} / {colsum.numel()} / {d.numel()} for N={N}, K={K}")
    _call(w, w, "am_ln_fold_weight", w.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
            _p(_need(bias, torch.float32, "bias")) if bias is not None else None, wf.data_ptr(), colsum.data_ptr(), d.data_ptr(), N, K)
    return wf, colsum, d


def layernorm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float = 1e-5,
              out: Optional[torch.Tensor] = None, stats_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """stats_out (rows, 2) fp32: also receives (mean, rstd) of the OUTPUT rows (for a linear that folds the next LayerNorm)."""
    _need(x, H16, "x"); _need(w, torch.float32, "w"); _need(b, torch.float32, "b")
    Cdim = x.shape[-1]
    rows = x.numel() // Cdim
    if out is None:
        out = torch.empty_like(x)
    if stats_out is not None:
        _call(x, x, "am_layernorm_stats_bf16", x.data_ptr(), out.data_ptr(), w.data_ptr(), b.data_ptr(),
                rows, Cdim, eps, _need(stats_out, torch.float32, "stats_out").data_ptr())
        return out
    _call(x, x, "am_layernorm_bf16", x.data_ptr(), out.data_ptr(), w.data_ptr(), b.data_ptr(),
                                      rows, Cdim, eps)
    return out


def add_layernorm_f32(h32: torch.Tensor, y: Optional[torch.Tensor] = None, w: Optional[torch.Tensor] = None,
                      b: Optional[torch.Tensor] = None, eps: float = 1e-5, out: Optional[torch.Tensor] = None,
                      dtype: Optional[torch.dtype] = None) -> Optional[torch.Tensor]:
    """am_add_layernorm_f32 - the fp32 residual stream of the reference's Stage II / DINOv2 encoder in one pass:
    h32 (rows, C) fp32 += y (rows, C) 16-bit (None: nothing to add), IN PLACE; returns LayerNorm(h32) * w + b rounded to the 16-bit type
    (`dtype`, or y's) for the next linear - or None when w is None (accumulate only)."""
    _need(h32, torch.float32, "h32")
    Cdim = h32.shape[-1]
    rows = h32.numel() // Cdim
    if y is not None:
        _need(y, H16, "y")
        assert y.numel() == h32.numel()
        dtype = y.dtype
    if w is None:
        assert y is not None, "add_layernorm_f32: nothing to do"
        _call(h32, dtype, "am_add_layernorm_f32", h32.data_ptr(), y.data_ptr(), None, None, None, rows, Cdim, eps)
        return None
    assert dtype in H16, "add_layernorm_f32: the 16-bit output type must be given when there is no branch to take it from"
    _need(w, torch.float32, "w"); _need(b, torch.float32, "b")
    if out is None:
        out = torch.empty(h32.shape, dtype=dtype, device=h32.device)
    _call(h32, dtype, "am_add_layernorm_f32", h32.data_ptr(), _p(y), _need(out, dtype, "out").data_ptr(),
            w.data_ptr(), b.data_ptr(), rows, Cdim, eps)
    return out


def _head_post_args(x: torch.Tensor, heads: int, kinds: Sequence[int], seq_len: int, rows_per_frame: int, w_q, w_k, rope, eps: float,
                    out_q, out_k, out_vt):
    """(AmHeadPostArgs of the head split of x (rows, heads * len(kinds) * 128), (Q, K, Vt)): the caller's outputs, or fresh ZERO-filled
    ones padded to the attention kernels' tiles for the kinds present (the pad rows and columns are read by the kernels)."""
    rows = x.shape[0]
    nseq = rows // seq_len
    sq_pad, sk_pad = round_up(seq_len, 256), round_up(seq_len, 64)
    h = L.AmHeadPostArgs()
    h.X = x.data_ptr(); h.ldx = x.stride(0)
    h.rows = rows; h.seq_len = seq_len; h.rows_per_frame = rows_per_frame
    h.heads = heads; h.nparts = len(kinds)
    for i, k in enumerate(kinds):
        h.kinds[i] = k
    h.w_q = _p(w_q); h.w_k = _p(w_k); h.eps = eps
    if rope is not None:
        h.rope_cos = _need(rope[0], torch.float32, "rope_cos").data_ptr()
        h.rope_sin = _need(rope[1], torch.float32, "rope_sin").data_ptr()
    if 0 in kinds and out_q is None:
        out_q = torch.zeros((nseq, heads, sq_pad, HEAD_DIM), dtype=x.dtype, device=x.device)
    if 1 in kinds and out_k is None:
        out_k = torch.zeros((nseq, heads, sk_pad, HEAD_DIM), dtype=x.dtype, device=x.device)
    if 2 in kinds and out_vt is None:
        out_vt = torch.zeros((nseq, heads, HEAD_DIM, sk_pad), dtype=x.dtype, device=x.device)
    h.out_q = _p(out_q); h.sq_pad = out_q.shape[2] if out_q is not None else 0
    h.out_k = _p(out_k); h.out_vt = _p(out_vt)
    h.sk_pad = out_k.shape[2] if out_k is not None else (out_vt.shape[3] if out_vt is not None else 0)
    return h, (out_q, out_k, out_vt)


def head_post(x: torch.Tensor, heads: int, kinds: Sequence[int], seq_len: int, rows_per_frame: int,
              w_q: Optional[torch.Tensor] = None, w_k: Optional[torch.Tensor] = None,
              rope: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, eps: float = 1e-6,
              out_q: Optional[torch.Tensor] = None, out_k: Optional[torch.Tensor] = None,
              out_vt: Optional[torch.Tensor] = None):
    """Split heads of x (rows, heads*len(kinds)*128), apply qk-RMSNorm (+RoPE), and write the
    attention operand layouts.  Returns (Q, K, Vt) (None for absent kinds):
      Q  (nseq, H, sq_pad, 128), K (nseq, H, sk_pad, 128), Vt (nseq, H, 128, sk_pad)."""
    _need_rows(x, H16, "x")
    h, outs = _head_post_args(x, heads, kinds, seq_len, rows_per_frame, w_q, w_k, rope, eps, out_q, out_k, out_vt)
    _call(x, x, "am_head_post", C.byref(h))
    return outs


def gemm_head_post(a: torch.Tensor, w: torch.Tensor, heads: int, kinds: Sequence[int], seq_len: int, rows_per_frame: int,
                   w_q: Optional[torch.Tensor] = None, w_k: Optional[torch.Tensor] = None,
                   rope: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, eps: float = 1e-6,
                   out_q: Optional[torch.Tensor] = None, out_k: Optional[torch.Tensor] = None,
                   out_vt: Optional[torch.Tensor] = None, x: Optional[torch.Tensor] = None,
                   bias: Optional[torch.Tensor] = None, ln: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, ablate: int = 0):
    """am_gemm_headpost_bf16: (a @ w.T) -> head split / qk-RMSNorm / RoPE / attention layouts in ONE launch; the arguments of `gemm`
    (no activation; `ln`: the LayerNorm folded into the projection, as gemm's) and of `head_post`.  `x` (rows, N) is the linear's output
    buffer the un-fused pair would use (only the tile grid's remainder rows are written to it).  Returns (Q, K, Vt) like head_post."""
    _need(a, H16, "a"); _need(w, a.dtype, "w")
    rows, K = a.shape
    N = w.shape[0]
    assert N == heads * len(kinds) * HEAD_DIM and w.shape[1] == K
    if x is None:
        x = torch.empty((rows, N), dtype=a.dtype, device=a.device)
    _need_rows(x, a.dtype, "x")
    g = L.AmGemmArgs()
    g.A1 = a.data_ptr(); g.lda1 = a.stride(0); g.K1 = K
    g.W = w.data_ptr(); g.ldw = w.stride(0)
    g.C = x.data_ptr(); g.ldc = x.stride(0)
    g.M, g.N, g.K = rows, N, K
    g.act = ablate & L.GEMM_ABLATE_MASK      # timing ablations of the fused epilogue (no Q / K rows, no V^T read-back); never on the product path
    _fold_args(g, bias, ln)
    h, outs = _head_post_args(x, heads, kinds, seq_len, rows_per_frame, w_q, w_k, rope, eps, out_q, out_k, out_vt)
    _call(a, a, "am_gemm_headpost_bf16", C.byref(g), C.byref(h))
    return outs


STATE_LD = L.ATTN_STATE_LD   # floats per row of a two-pass attention state: O[128], m, l, pad


def _attn_args(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, sq: int, sk: int, out: Optional[torch.Tensor], nchunks: int,
               scale: Optional[float], defer_log2: int, rows: int, state_mode: int, state: Optional[torch.Tensor], chunk_first: int,
               chunk_total: int):
    """(AmAttnArgs, out) of an attention over the operand layouts of `attention`; `defer_log2` is the field as each kernel family reads it."""
    _need(q, H16, "q"); _need(k, q.dtype, "k"); _need(vt, q.dtype, "vt")
    nseq, H, sq_pad, _ = q.shape
    sk_pad = k.shape[-2]
    if out is None:
        out = torch.empty((nseq * sq, H * HEAD_DIM), dtype=q.dtype, device=q.device)
    _need_rows(out, q.dtype, "out")
    a = L.AmAttnArgs()
    a.Q, a.K, a.Vt, a.O = q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr()
    a.nseq, a.heads, a.sq, a.sq_pad, a.sk, a.sk_pad = nseq, H, sq, sq_pad, sk, sk_pad
    a.nchunks = nchunks
    a.chunk_stride = nseq * H * sk_pad * HEAD_DIM
    a.ldo = out.stride(0)
    a.scale = scale if scale is not None else HEAD_DIM ** -0.5
    a.defer_log2 = defer_log2
    a.rows, a.state_mode, a.chunk_first, a.chunk_total = rows, state_mode, chunk_first, chunk_total
    if state is not None:
        _need(state, torch.float32, "state")
        assert state.numel() >= nseq * H * sq_pad * STATE_LD
        a.state = state.data_ptr()
    return a, out


def attention(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, sq: int, sk: int,
              out: Optional[torch.Tensor] = None, nchunks: int = 1, defer_log2: int = L.ATTN_REBASE_DEFERRED,
              scale: Optional[float] = None, rows: int = 0, state_mode: int = 0,
              state: Optional[torch.Tensor] = None, chunk_first: int = 0, chunk_total: int = 0) -> torch.Tensor:
    """softmax(q k^T * scale) v on pre-laid-out operands.
      q (nseq, H, sq_pad, 128); k ([chunks,] nseq, H, sk_pad, 128); vt ([chunks,] nseq, H, 128, sk_pad)
      -> out (nseq * sq, H * 128)
    Two-pass form (am_attn_args in include/actionmesh_amd.h): `rows` selects the query blocks (1 = the full blocks,
    2 = the rest), `state_mode` 1 saves / 2 resumes the (O, m, l) of the full blocks in `state`
    (nseq * H, sq_pad, STATE_LD) fp32, and the chunks walked are (chunk_first + i) % chunk_total."""
    a, out = _attn_args(q, k, vt, sq, sk, out, nchunks, scale, defer_log2, rows, state_mode, state, chunk_first, chunk_total)
    _call(q, q, "am_attention_bf16", C.byref(a))
    return out


def _quantize_fp8(a, q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor,
                  quantize_out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """am_attention_quantize_fp8 for the call `a` describes -> uint8 (q8, k8, vt8): the caller's `quantize_out`, or fresh tensors."""
    if quantize_out is not None:
        q8, k8, vt8 = (_need(t, torch.uint8, "quantize_out") for t in quantize_out)
        if q8.shape != q.shape or k8.shape != k.shape or vt8.shape != vt.shape:
            raise ValueError("attention_fp8: quantize_out must have the shapes of q, k, vt")
    else:
        q8 = torch.empty(q.shape, dtype=torch.uint8, device=q.device)
        k8 = torch.empty(k.shape, dtype=torch.uint8, device=q.device)
        vt8 = torch.empty(vt.shape, dtype=torch.uint8, device=q.device)
    _call(q, q, "am_attention_quantize_fp8", C.byref(a), q8.data_ptr(), k8.data_ptr(), vt8.data_ptr())
    return q8, k8, vt8


def attention_fp8(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, sq: int, sk: int,
                  out: Optional[torch.Tensor] = None, nchunks: int = 1, scale: Optional[float] = None,
                  quantized: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None, ablate: int = 0,
                  rows: int = 0, state_mode: int = 0, state: Optional[torch.Tensor] = None, chunk_first: int = 0,
                  chunk_total: int = 0, quantize_out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None,
                  **_ignored) -> torch.Tensor:
    """fp8 (e4m3) attention on the bf16 operand layouts of `attention`: quantise (unless `quantized` = (q8, k8, vt8) from an
    earlier call is passed), then QK^T / P.V on the MX-scaled fp8 MFMA.  Returns out (nseq * sq, H * 128) bf16.
    rows / state_mode / state / chunk_first / chunk_total: the two-pass forms, as in `attention`.  `quantize_out`: caller-owned uint8
    (q8, k8, vt8) of the shapes of q / k / vt that receive the quantisation (default: fresh tensors)."""
    # defer_log2 carries the timing ablations of the fp8 kernel (tools/kernel_bench.py)
    a, out = _attn_args(q, k, vt, sq, sk, out, nchunks, scale, L.ATTN_FP8_ABLATE + ablate if ablate else 0, rows, state_mode, state, chunk_first,
                        chunk_total)
    q8, k8, vt8 = _quantize_fp8(a, q, k, vt, quantize_out) if quantized is None else quantized
    _call(q, q, "am_attention_fp8", C.byref(a), q8.data_ptr(), k8.data_ptr(), vt8.data_ptr())
    attention_fp8.last_quantized = (q8, k8, vt8)
    return out


def attention_quantize_fp8(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, sq: int, sk: int,
                           quantize_out: Tuple[torch.Tensor, torch.Tensor, torch.Tensor], nchunks: int = 1,
                           scale: Optional[float] = None, rows: int = 0, chunk_first: int = 0, chunk_total: int = 0) -> None:
    """The quantiser of `attention_fp8` on its own, into the caller's uint8 (q8, k8, vt8).  Only the chunks (chunk_first + i) %
    chunk_total, i < nchunks, are written (chunk_total = 0: chunks 0 .. nchunks - 1), and rows = 2 leaves q8 alone - as an attention
    call with the same arguments reads them."""
    a, _ = _attn_args(q, k, vt, sq, sk, None, nchunks, scale, 0, rows, 0, None, chunk_first, chunk_total)
    _quantize_fp8(a, q, k, vt, quantize_out)


def attention_fallback_count() -> int:
    """Workgroups the exact fallback of the lazy attention kernel has recomputed so far on the current device."""
    n = C.c_uint64(0)
    L.check(L.lib().am_attention_fallback_count(C.byref(n)), "am_attention_fallback_count")
    return int(n.value)


def f32_to_bf16(x: torch.Tensor, dtype=torch.bfloat16, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 -> the 16-bit type (round to nearest even); `dtype=torch.float16` runs the float16 build of the library."""
    _need(x, torch.float32, "x")
    y = torch.empty(x.shape, dtype=dtype, device=x.device) if out is None else _need(out, dtype, "out")
    if y.numel() != x.numel():
        raise ValueError(f"f32_to_bf16: out has {y.numel()} elements for {x.numel()} inputs")
    _call(x, dtype, "am_f32_to_bf16", x.data_ptr(), y.data_ptr(), x.numel())
    return y


def timestep_sinusoid(t: torch.Tensor, width: int, dtype=torch.bfloat16, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """t (rows,) fp32 -> 16-bit (rows, width): [sin | cos] of t * 10000^(-i / (width / 2)); `dtype=torch.float16` runs the float16 build."""
    _need(t, torch.float32, "t")
    y = torch.empty((t.numel(), width), dtype=dtype, device=t.device) if out is None else _need(out, dtype, "out")
    if tuple(y.shape) != (t.numel(), width):
        raise ValueError(f"timestep_sinusoid: out {tuple(y.shape)} != ({t.numel()}, {width})")
    _call(t, dtype, "am_timestep_sinusoid", t.data_ptr(), y.data_ptr(), t.numel(), width)
    return y


def _point_embed(what: str, key, out_dtype, query, in_channels, extra_channels, num_freqs, include_pi, ld_out, out) -> torch.Tensor:
    """point_embed / point_embed_f32 behind their checks: entry point am_<what> of the build `key` picks, output of `out_dtype`."""
    rows = query.shape[0]
    out = _out_rows(out, rows, ld_out, out_dtype, query.device, what)
    _call(query, key, "am_" + what, query.data_ptr(), query.stride(0), rows, in_channels, extra_channels, num_freqs, int(include_pi),
          out.data_ptr(), ld_out)
    return out


def _patchify(what: str, key, out_dtype, pixels, patch, ld_out, out) -> torch.Tensor:
    T, Cin, H, W = pixels.shape
    out = _out_rows(out, T * (H // patch) * (W // patch), ld_out, out_dtype, pixels.device, what)
    _call(pixels, key, "am_" + what, pixels.data_ptr(), T, Cin, H, W, patch, out.data_ptr(), ld_out)
    return out


def _displacement(what: str, key, logits, out_dim, out) -> torch.Tensor:
    _call(logits, key, "am_" + what, logits.data_ptr(), logits.stride(0), logits.shape[0], out_dim, out.data_ptr())
    return out


def point_embed(query: torch.Tensor, in_channels: int, extra_channels: int, num_freqs: int, include_pi: bool,
                ld_out: int = 64, dtype=torch.bfloat16, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """query (rows, >= in+extra) fp32, rows may be strided -> 16-bit (rows, ld_out): FrequencyPositionalEmbedding + extras, zero padded."""
    _need_rows(query, torch.float32, "query")
    return _point_embed("point_embed", dtype, dtype, query, in_channels, extra_channels, num_freqs, include_pi, ld_out, out)


def patchify(pixels: torch.Tensor, patch: int, ld_out: int, dtype=torch.bfloat16, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pixels (T, C, H, W) fp32 -> 16-bit (T * (H // patch) * (W // patch), ld_out): rows of the kernel = stride patch
    convolution in flattened-Conv2d-weight column order, zero padded."""
    _need(pixels, torch.float32, "pixels")
    return _patchify("patchify", dtype, dtype, pixels, patch, ld_out, out)


def displacement(logits: torch.Tensor, out_dim: int, out: torch.Tensor) -> torch.Tensor:
    """out (rows, out_dim) fp32 = 2 sigmoid(-logits[:, :out_dim]) - 1."""
    _need_rows(logits, H16, "logits"); _need(out, torch.float32, "out")
    return _displacement("displacement", logits, logits, out_dim, out)


def flow_step(v: torch.Tensor, latents: torch.Tensor, scales: Sequence[float], dt: float,
              is_additive: bool, unobserved: Optional[Sequence[bool]]) -> None:
    """In place: latents (T, N, D) fp32 += sign * bf16(dt * cfg(v)); v (n_branches, T, N, D) bf16 (or float16: that build's rounding).
    An fp32 velocity - an exact-fp32 model's - takes am_flow_step_f32: the reference's fp32 arithmetic, nothing rounded to 16 bits."""
    if v.dtype == torch.float32:
        return flow_step_f32(v, latents, scales, dt, is_additive, unobserved)
    _need(v, H16, "v"); _need(latents, torch.float32, "latents")
    nb, T, N, D = v.shape
    sc = (C.c_float * max(1, len(scales)))(*[float(s) for s in scales])
    un = None
    if unobserved is not None:
        un = (C.c_uint8 * T)(*[1 if u else 0 for u in unobserved])
    _call(v, v, "am_flow_step", v.data_ptr(), latents.data_ptr(), nb, sc, float(dt), 1 if is_additive else 0,
                                 un, T, N, D)


NO_NEIGHBOUR_TEXT = "nearest_neighbors: a query has no finite distance to any point (NaN / inf coordinates in the inputs)"


def _cloud(who: str, t: torch.Tensor, name: str, dims=(2, 3)) -> int:
    """The check every cloud of the point searches passes: a contiguous fp32 device tensor (n, 3) - or (B, n, 3) where `dims` allows it -
    that is not empty (no points, or a batch of 0).  Returns n."""
    _need(t, torch.float32, name)
    if t.dim() not in dims or t.shape[-1] != 3:
        raise ValueError(f"{who}: expected (..., n, 3) {name}, got {tuple(t.shape)}")
    if 0 in t.shape:
        raise ValueError(f"{who}: empty point cloud")
    return t.shape[-2]


def _nn_outputs(who: str, queries: torch.Tensor, point_batch: Optional[int], precise: bool):
    """(batch, index int32, d2) of a search: `point_batch` is the points' (or the grid's) batch, None when one cloud serves every
    batch entry.  A 3-D operand sets the batch and the outputs are (batch, Q); with none they are (Q,)."""
    batch = queries.shape[0] if queries.dim() == 3 else None
    if point_batch is not None and batch not in (None, point_batch):
        raise ValueError(f"{who}: points batch {point_batch} != queries batch {batch}")
    batch = point_batch if batch is None else batch
    shape = (queries.shape[-2],) if batch is None else (batch, queries.shape[-2])
    return (1 if batch is None else batch, torch.empty(shape, dtype=torch.int32, device=queries.device),
            torch.empty(shape, dtype=torch.float64 if precise else torch.float32, device=queries.device))


def _nn_valid(flags: Sequence[torch.Tensor], indices: Sequence[torch.Tensor]) -> None:
    """The check behind the searches, ONE device-to-host read for any number of grid flag words and index tensors: a raised flag or an
    index -1 - the kernels' candidate rules never take a NaN distance, and -1 would wrap in a later gather - is an error.  Every raised
    flag is consumed and named by the one error, so none is left to fire on a later check."""
    words = [f.view(1) for f in flags] + [(i < 0).any().view(1) for i in indices]
    got = (words[0] if len(words) == 1 else torch.cat(words)).tolist() if words else []      # one word: no launch beside its own
    bits = 0
    for f, word in zip(flags, got):
        if word:
            f.zero_()
            bits |= word
    if bits:
        raise ValueError(f"nn_grid_search: bad grid ({', '.join(t for b, t in _NN_GRID_FLAGS.items() if bits & b)})")
    if any(got[len(flags):]):
        raise ValueError(NO_NEIGHBOUR_TEXT)


def nearest_neighbors(points: torch.Tensor, queries: torch.Tensor, precise: bool = True,
                      check: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """am_nn_search: for every query its nearest point (exact, brute force).  points (P, 3) or (B, P, 3) fp32, queries
    (Q, 3) or (B, Q, 3) fp32 (a 2-D operand beside a 3-D one is shared by the batch).  Returns (index int32, SQUARED
    distance: float64 when `precise` - the KD-tree arithmetic of actionbench/chamfer.py - else float32), shaped like the
    queries minus the coordinate axis.
    `check` (default): one device-to-host read behind the search that turns "no finite distance" (index -1) into an error.
    Callers inside a loop of searches (the ICP: 4800 of them) pass check=False and validate once per batch instead
    (`nn_indices_valid`), so the stream is not serialised per search."""
    P, Q = _cloud("nearest_neighbors", points, "points"), _cloud("nearest_neighbors", queries, "queries")
    batch, idx, d2 = _nn_outputs("nearest_neighbors", queries, points.shape[0] if points.dim() == 3 else None, precise)
    ws, need = _workspace(queries.device, "am_nn_workspace_bytes", P, Q, batch, 1 if precise else 0, at_least=1)
    a = L.AmNnArgs()
    a.points, a.n_points, a.points_bstride = points.data_ptr(), P, (P * 3 if points.dim() == 3 else 0)
    a.queries, a.n_queries, a.queries_bstride = queries.data_ptr(), Q, (Q * 3 if queries.dim() == 3 else 0)
    a.batch, a.precise = batch, 1 if precise else 0
    a.out_index, a.out_d2 = idx.data_ptr(), d2.data_ptr()
    _call(queries, None, "am_nn_search", C.byref(a), ws.data_ptr(), need)
    if check:
        _nn_valid((), (idx,))
    return idx, d2


def nn_indices_valid(*indices: torch.Tensor) -> None:
    """The deferred form of nearest_neighbors' check: ONE device-to-host read for any number of index tensors."""
    _nn_valid((), indices)


class IcpState:
    """What am_icp_step keeps between the iterations of one ICP call, allocated once: params (B, 12) fp32 = [T, d6, s] at the
    reference's start (T = 0, d6 = (1, 0, 0, 0, 1, 0), s = 1), Adam's adam_m and adam_v (B, 12) fp32 at 0, best (16) fp32 =
    [R, T, s, loss] with the loss at +inf, the outputs of the last step - out_loss (B,), out_rot (B, 9), and out_sums (B, 2, 13) /
    out_grad (B, 12) fp64 once a step has asked for them - the flag word, and the workspace, sized on the first step and reused while
    the cloud sizes stay.  Every tensor may be replaced by a caller's buffer of the same shape and dtype."""

    def __init__(self, batch: int, device):
        if batch < 1:
            raise ValueError(f"IcpState: batch {batch} < 1")
        self.batch, self.device = int(batch), torch.device(device)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.params = torch.tensor([0.0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 1, 1], **f32).repeat(batch, 1)
        self.adam_m, self.adam_v = torch.zeros((batch, 12), **f32), torch.zeros((batch, 12), **f32)
        self.best = torch.zeros((16,), **f32)
        self.best[15] = float("inf")
        self.out_loss, self.out_rot = torch.zeros((batch,), **f32), torch.zeros((batch, 9), **f32)
        self.out_sums: Optional[torch.Tensor] = None
        self.out_grad: Optional[torch.Tensor] = None
        self.out_flag = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self.workspace: Optional[torch.Tensor] = None
        self.workspace_bytes = 0              # am_icp_workspace_bytes of the sizes of `_sized_for`
        self._sized_for = None


def icp_step(state: IcpState, pred: torch.Tensor, gt: torch.Tensor, rot_init: torch.Tensor, t: int, lr: float = 0.01,
             betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, update: bool = True, return_sums: bool = False) -> IcpState:
    """am_icp_step: iteration `t` (1, 2, ...: Adam's step count) of the ICP on pred (P, 3), gt (Q, 3) and rot_init (B, 3, 3) or (B, 9)
    fp32, in place on `state`; no device-to-host read.  `update=False` computes the outputs and leaves params, adam_m, adam_v and best
    as they are.  `return_sums` also fills state.out_sums and state.out_grad (fp64).  state.out_flag collects L.ICP_NO_NEIGHBOUR over
    the steps: the caller reads it when it likes."""
    P, Q, B = _cloud("icp_step", pred, "pred", dims=(2,)), _cloud("icp_step", gt, "gt", dims=(2,)), state.batch
    _need(rot_init, torch.float32, "rot_init")
    if tuple(rot_init.shape) not in ((B, 3, 3), (B, 9)):
        raise ValueError(f"icp_step: rot_init {tuple(rot_init.shape)} does not hold the state's {B} candidates")
    if int(t) < 1:
        raise ValueError(f"icp_step: step count {t} < 1")
    want = {"params": (B, 12), "adam_m": (B, 12), "adam_v": (B, 12), "best": (16,), "out_loss": (B,), "out_rot": (B, 9)}
    for name, shape in want.items():
        ten = _need(getattr(state, name), torch.float32, f"state.{name}")
        if tuple(ten.shape) != shape:
            raise ValueError(f"icp_step: state.{name} {tuple(ten.shape)} != {shape}")
    _need(state.out_flag, torch.int32, "state.out_flag")
    for ten in (gt, rot_init, state.params, state.adam_m, state.adam_v, state.best, state.out_loss, state.out_rot, state.out_flag):
        if ten.device != pred.device:
            raise ValueError("icp_step: the clouds, rot_init and the state are on different devices")
    if return_sums:
        if state.out_sums is None:
            state.out_sums = torch.zeros((B, 2, 13), dtype=torch.float64, device=pred.device)
        if state.out_grad is None:
            state.out_grad = torch.zeros((B, 12), dtype=torch.float64, device=pred.device)
        for name, shape in (("out_sums", (B, 2, 13)), ("out_grad", (B, 12))):
            ten = _need(getattr(state, name), torch.float64, f"state.{name}")
            if tuple(ten.shape) != shape or ten.device != pred.device:
                raise ValueError(f"icp_step: state.{name} {tuple(ten.shape)} != {shape} on the clouds' device")
    if state._sized_for != (P, Q):
        need = _entry(None, "am_icp_workspace_bytes")[1](P, Q, B)
        if state.workspace is None or state.workspace.numel() < need:
            state.workspace = torch.empty((max(need, 8),), dtype=torch.uint8, device=pred.device)
        state.workspace_bytes, state._sized_for = need, (P, Q)
    _need(state.workspace, torch.uint8, "state.workspace")
    a = L.AmIcpArgs()
    a.pred, a.gt, a.rot_init, a.n_pred, a.n_gt, a.batch = pred.data_ptr(), gt.data_ptr(), rot_init.data_ptr(), P, Q, B
    a.update = 1 if update else 0
    a.params, a.adam_m, a.adam_v, a.best = state.params.data_ptr(), state.adam_m.data_ptr(), state.adam_v.data_ptr(), state.best.data_ptr()
    a.lr, a.beta1, a.beta2, a.eps = float(lr), float(betas[0]), float(betas[1]), float(eps)
    a.bias_correction1, a.bias_correction2 = 1.0 - float(betas[0]) ** int(t), 1.0 - float(betas[1]) ** int(t)
    a.out_loss, a.out_rot, a.out_flag = state.out_loss.data_ptr(), state.out_rot.data_ptr(), state.out_flag.data_ptr()
    if return_sums:
        a.out_sums, a.out_grad = state.out_sums.data_ptr(), state.out_grad.data_ptr()
    _call(pred, None, "am_icp_step", C.byref(a), state.workspace.data_ptr(), min(state.workspace_bytes, state.workspace.numel()))
    return state


class NnGrid:
    """The uniform grid of one cloud or of a batch of clouds (am_nn_grid of include/actionmesh_amd.h): ONE device allocation of
    am_nn_grid_bytes carved into frame (B, 8) fp32, slabs (B, 2, 3, G) fp32, cell_start (B, G^3 + 2) int32, order (B, P) int32 and
    sorted (B, P, 4) fp32.  `shared`: built from a 2-D cloud - a search of any batch uses the one grid.  `order` is the cloud's own
    cell order: the `query_order` to pass when this cloud is the QUERY of another grid.  `buffer`: the caller's allocation of exactly
    am_nn_grid_bytes to carve instead of a fresh one."""

    def __init__(self, n_points: int, batch: int, cells: int, shared: bool, device, buffer: Optional[torch.Tensor] = None):
        self.n_points, self.batch, self.cells, self.shared, self.device = n_points, batch, cells, shared, device
        nbytes = _entry(None, "am_nn_grid_bytes")[1](n_points, batch, cells)
        if nbytes == 0:
            raise ValueError(f"nn_grid_build: no grid of {cells} cells per axis over {batch} x {n_points} points (cells 1 .. {L.NN_GRID_MAX_CELLS})")
        if buffer is not None and (buffer.dtype != torch.uint8 or buffer.numel() != nbytes or not buffer.is_contiguous() or buffer.data_ptr() % 16):
            raise ValueError(f"NnGrid: the buffer must be {nbytes} contiguous, 16-byte aligned uint8 elements")
        self.buffer = torch.empty((nbytes,), dtype=torch.uint8, device=device) if buffer is None else buffer
        off = 0

        def carve(shape, dtype):
            nonlocal off
            n = 4
            for s in shape:
                n *= s
            t = self.buffer[off:off + n].view(dtype).view(shape)
            off += round_up(n, 16)
            return t

        self.frame = carve((batch, 8), torch.float32)
        self.slabs = carve((batch, 2, 3, cells), torch.float32)
        self.cell_start = carve((batch, cells ** 3 + 2), torch.int32)
        self.order = carve((batch, n_points), torch.int32)
        self.sorted = carve((batch, n_points, 4), torch.float32)
        assert off == nbytes
        self.flags = torch.zeros((1,), dtype=torch.int32, device=device)      # every flag a check=False search has raised since valid()

    def struct(self) -> "L.AmNnGrid":
        g = L.AmNnGrid()
        g.n_points, g.batch, g.cells = self.n_points, self.batch, self.cells
        g.frame, g.slabs, g.cell_start = self.frame.data_ptr(), self.slabs.data_ptr(), self.cell_start.data_ptr()
        g.order, g.sorted = self.order.data_ptr(), self.sorted.data_ptr()
        return g


_NN_GRID_FLAGS = {L.NN_GRID_BAD_ORDER: "an order entry outside the points", L.NN_GRID_BAD_CELL_START: "cell_start not ascending inside the points",
                  L.NN_GRID_BAD_INDEX: "a sorted record with an index outside the points", L.NN_GRID_BAD_QUERY_ORDER: "a query_order entry outside the queries"}


def nn_grid_default_cells(n_points: int) -> int:
    """G = clamp(ceil(cbrt(2 P)), 1, 128): about half a point per cell (tools/nn_grid_timing.py sweeps it)."""
    g = max(1, int(round((2.0 * n_points) ** (1.0 / 3.0))))
    while g ** 3 < 2 * n_points:
        g += 1
    while g > 1 and (g - 1) ** 3 >= 2 * n_points:
        g -= 1
    return min(max(g, 1), L.NN_GRID_MAX_CELLS)


def nn_grid_build(points: torch.Tensor, cells: Optional[int] = None) -> NnGrid:
    """am_nn_grid_cells + a stable torch sort + am_nn_grid_build: the grid of points (P, 3) - one shared grid - or (B, P, 3) fp32."""
    P = _cloud("nn_grid_build", points, "points")
    batch = points.shape[0] if points.dim() == 3 else 1
    G = nn_grid_default_cells(P) if cells is None else int(cells)
    if not 1 <= G <= L.NN_GRID_MAX_CELLS:
        raise ValueError(f"nn_grid_build: cells {G} outside 1 .. {L.NN_GRID_MAX_CELLS}")
    grid = NnGrid(P, batch, G, points.dim() == 2, points.device)
    ws, need = _workspace(points.device, "am_nn_grid_workspace_bytes", P, batch, G)
    cell = torch.empty((batch, P), dtype=torch.int32, device=points.device)
    flag = torch.empty((1,), dtype=torch.int32, device=points.device)
    a = L.AmNnGridBuildArgs()
    a.points, a.points_bstride, a.grid = points.data_ptr(), (P * 3 if points.dim() == 3 else 0), grid.struct()
    a.out_cell, a.out_flag, a.workspace, a.workspace_bytes = cell.data_ptr(), flag.data_ptr(), ws.data_ptr(), need
    _call(points, None, "am_nn_grid_cells", C.byref(a))
    grid.order.copy_(torch.sort(cell, dim=1, stable=True).indices)          # plumbing: (cell, index) order
    _call(points, None, "am_nn_grid_build", C.byref(a))
    return grid


def nn_grid_search(grid: NnGrid, queries: torch.Tensor, precise: bool = True, query_order: Optional[torch.Tensor] = None,
                   check: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """am_nn_grid_search: nearest_neighbors' (index int32, squared distance) bit for bit, through `grid`.  queries (Q, 3) or (B, Q, 3)
    fp32; a batched grid needs the same B (2-D queries are then shared).  `query_order`: int32 (Q,) or (B, Q), a permutation of the
    queries - the order in which lanes pick them (the query cloud's own NnGrid.order makes a wave share cells); results stay at the
    query's own position.  `check` as in nearest_neighbors; with check=False the kernel's flag is kept in grid.flags for nn_grid_valid."""
    Q = _cloud("nn_grid_search", queries, "queries")
    if queries.device != grid.device:
        raise ValueError("nn_grid_search: the queries and the grid are on different devices")
    batch, idx, d2 = _nn_outputs("nn_grid_search", queries, None if grid.shared else grid.batch, precise)
    flag = torch.empty((1,), dtype=torch.int32, device=queries.device)
    a = L.AmNnGridSearchArgs()
    a.grid = grid.struct()
    a.queries, a.n_queries, a.queries_bstride = queries.data_ptr(), Q, (Q * 3 if queries.dim() == 3 else 0)
    a.batch, a.precise = batch, 1 if precise else 0
    if query_order is not None:
        _need(query_order, torch.int32, "query_order")
        if tuple(query_order.shape) not in ((Q,), (1, Q), (batch, Q)):
            raise ValueError(f"nn_grid_search: query_order {tuple(query_order.shape)} is neither ({Q},) nor ({batch}, {Q})")
        a.query_order, a.query_order_bstride = query_order.data_ptr(), (Q if query_order.dim() == 2 and query_order.shape[0] == batch and batch > 1 else 0)
    a.out_index, a.out_d2, a.out_flag = idx.data_ptr(), d2.data_ptr(), flag.data_ptr()
    _call(queries, None, "am_nn_grid_search", C.byref(a))
    if check:
        _nn_valid((flag,), (idx,))
    else:
        grid.flags |= flag
    return idx, d2


def nn_grid_valid(grids: Sequence[NnGrid], *indices: torch.Tensor) -> None:
    """The deferred check of check=False grid searches: ONE device-to-host read for the flags of `grids` and any number of index tensors."""
    _nn_valid([g.flags for g in grids], indices)


def nearest_neighbors_grid(points: torch.Tensor, queries: torch.Tensor, precise: bool = True,
                           check: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """nearest_neighbors through a grid built for the call (default cells): the same operands, return types, bits and exception types
    (the shape and batch errors are nn_grid_build's and nn_grid_search's, and name them)."""
    return nn_grid_search(nn_grid_build(points), queries, precise=precise, check=check)


_FPS_DTYPES = {torch.float32: L.FPS_F32, torch.float16: L.FPS_F16, torch.bfloat16: L.FPS_BF16}


def farthest_point_sample(points: torch.Tensor, n_samples: int, start_idx=None, dist_dims: Optional[int] = None,
                          return_dist: bool = False, check: bool = True, threads: int = 0):
    """am_fps: exact greedy farthest-point sampling (the contract is the header's).  points (N, D) or (B, N, D), fp32 / fp16 / bf16,
    D = 1..8, any strides whose channel axis is contiguous (x[..., :3] of a wider tensor is passed as it is, no copy).  The first
    `dist_dims` channels enter the distance (default: all D).  `start_idx`: None (every cloud starts at point 0), an int, or an
    integer tensor (B,).  Returns the int32 indices (B, n_samples) - (n_samples,) for a 2-D input - and with `return_dist` also
    the fp32 squared distance each point had to the set chosen before it (+inf for the first).
    `check` (default): one device-to-host read in front of the launch - every coordinate finite, every start index in range.
    A caller that knows its inputs passes check=False and nothing serialises the stream.  `threads`: 0 = the library's choice of
    workgroup size, 256 / 512 / 1024 for benchmarks (tools/kernel_bench.py fps)."""
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise RuntimeError("farthest_point_sample: actionmesh_amd kernels need a device tensor (no CPU path)")
    if points.dtype not in _FPS_DTYPES:
        raise TypeError(f"farthest_point_sample: expected float32, float16 or bfloat16 points, got {points.dtype}")
    if points.dim() not in (2, 3):
        raise ValueError(f"farthest_point_sample: expected (N, D) or (B, N, D) points, got {tuple(points.shape)}")
    p3 = points if points.dim() == 3 else points.unsqueeze(0)
    B, N, D = p3.shape
    dd = D if dist_dims is None else int(dist_dims)
    K = int(n_samples)
    if B < 1 or N < 1:
        raise ValueError(f"farthest_point_sample: empty point cloud {tuple(points.shape)}")
    if not 1 <= D <= 8 or not 1 <= dd <= D:
        raise ValueError(f"farthest_point_sample: needs 1 <= dist_dims ({dd}) <= D ({D}) <= 8")
    if not 1 <= K <= N:
        raise ValueError(f"farthest_point_sample: n_samples {K} outside 1 .. N ({N})")
    sb, sp, sc = p3.stride()
    if N == 1:
        sp = D
    if B == 1:
        sb = 0
    if (D > 1 and sc != 1) or sp < D or sb < 0:
        raise ValueError(f"farthest_point_sample: the channel axis must be contiguous and points must not overlap (strides {p3.stride()})")
    dev = p3.device
    start = None
    if start_idx is not None:
        start = torch.as_tensor(start_idx, device=dev)
        if start.is_floating_point() or start.dtype == torch.bool:
            raise TypeError(f"farthest_point_sample: start_idx must hold integers, got {start.dtype}")
        start = start.reshape(-1).expand(B) if start.numel() == 1 else start.reshape(-1)
        if start.numel() != B:
            raise ValueError(f"farthest_point_sample: start_idx has {start.numel()} entries for a batch of {B}")
        if check and bool(((start < 0) | (start >= N)).any()):
            raise ValueError(f"farthest_point_sample: start_idx outside [0, {N})")
        start = start.to(torch.int32).contiguous()
    if check and not bool(torch.isfinite(p3[..., :dd]).all()):
        raise ValueError("farthest_point_sample: non-finite coordinates in the points")
    idx = torch.empty((B, K), dtype=torch.int32, device=dev)
    dist = torch.empty((B, K), dtype=torch.float32, device=dev) if return_dist else None
    ws, need = _workspace(dev, "am_fps_workspace_bytes", N, B, dd)
    a = L.AmFpsArgs()
    a.points, a.dtype, a.batch, a.n_points = p3.data_ptr(), _FPS_DTYPES[points.dtype], B, N
    a.dims, a.dist_dims, a.batch_stride, a.point_stride, a.n_samples = D, dd, sb, sp, K
    a.start_idx = start.data_ptr() if start is not None else None
    a.out_index, a.out_dist = idx.data_ptr(), (dist.data_ptr() if return_dist else None)
    a.workspace, a.workspace_bytes, a.threads = _p(ws), need, int(threads)
    _call(p3, None, "am_fps", C.byref(a))
    if points.dim() == 2:
        idx, dist = idx[0], (dist[0] if return_dist else None)
    return (idx, dist) if return_dist else idx


# ---- image preprocessing (csrc/am_image.hip; the contract is the header's, the geometry and the tables are image_preprocess.py's) ----
def image_alpha_stats(rgba: torch.Tensor) -> torch.Tensor:
    """am_image_alpha_stats: rgba (T, H, W, 4) uint8 -> int32 (T, 8) = [count(alpha > 127), min col, min row, max col, max row of
    alpha > 0, 0, 0, 0] per frame, on the device (the caller reads it)."""
    _need(rgba, torch.uint8, "image_alpha_stats: rgba")
    if rgba.dim() != 4 or rgba.shape[-1] != 4 or rgba.numel() == 0:
        raise ValueError(f"image_alpha_stats: expected non-empty (T, H, W, 4) uint8 frames, got {tuple(rgba.shape)}")
    stats = torch.empty((rgba.shape[0], 8), dtype=torch.int32, device=rgba.device)
    a = L.AmImageAlphaStatsArgs()
    a.rgba, a.n_frames, a.height, a.width, a.out_stats = rgba.data_ptr(), rgba.shape[0], rgba.shape[1], rgba.shape[2], stats.data_ptr()
    _call(rgba, None, "am_image_alpha_stats", C.byref(a))
    return stats


def _image_src(a, src: torch.Tensor, channels: int, composite: Optional[torch.Tensor], fill: int, frames, frames_dev: torch.Tensor) -> None:
    """The fields am_image_resample_args and am_image_materialize_args share.  `frames`: a ctypes array of AmImageFrame (host);
    `frames_dev`: the same bytes on the device."""
    _need(src, torch.uint8, "image: src")
    _need(frames_dev, torch.uint8, "image: frames_dev")
    if frames_dev.numel() != C.sizeof(frames):
        raise ValueError("image: frames_dev is not a copy of frames")
    if channels == 4:
        if composite is None:
            raise ValueError("image: an RGBA source needs the composite table")
        _need(composite, torch.uint8, "image: composite")
        if composite.numel() != 65536:
            raise ValueError(f"image: the composite table has 65536 entries, got {composite.numel()}")
    a.src, a.src_bytes, a.src_channels, a.fill = src.data_ptr(), src.numel(), int(channels), int(fill)
    a.composite = composite.data_ptr() if channels == 4 else None
    a.n_frames, a.frames, a.frames_dev = len(frames), C.addressof(frames), frames_dev.data_ptr()


def image_resample(src: torch.Tensor, channels: int, frames, frames_dev: torch.Tensor, taps, taps_dev: torch.Tensor, out_h: int,
                   out_w: int, composite: Optional[torch.Tensor] = None, fill: int = 255, norm_table: Optional[torch.Tensor] = None,
                   want_u8: bool = False) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """am_image_resample over frames described by `frames` (ctypes array of AmImageFrame) with the int32 tap tables `taps` (a
    contiguous numpy array; `taps_dev` its device copy).  Returns (pixel_values (T, 3, out_h, out_w) fp32 or None without a
    norm_table, the uint8 crop (T, out_h, out_w, 3) or None unless `want_u8`)."""
    T = len(frames)
    if norm_table is None and not want_u8:
        raise ValueError("image_resample: nothing to compute (no norm_table and want_u8=False)")
    _need(taps_dev, torch.int32, "image_resample: taps_dev")
    if taps.dtype.name != "int32" or not taps.flags["C_CONTIGUOUS"] or taps.size != taps_dev.numel():
        raise ValueError("image_resample: taps must be a contiguous int32 array and taps_dev its copy")
    a = L.AmImageResampleArgs()
    _image_src(a, src, channels, composite, fill, frames, frames_dev)
    a.out_w, a.out_h = int(out_w), int(out_h)
    a.taps, a.taps_dev, a.taps_len = taps.ctypes.data, taps_dev.data_ptr(), taps.size
    pix = u8 = None
    if norm_table is not None:
        _need(norm_table, torch.float32, "image_resample: norm_table")
        if norm_table.numel() != 768:
            raise ValueError(f"image_resample: the normalisation table is (3, 256), got {tuple(norm_table.shape)}")
        pix = torch.empty((T, 3, out_h, out_w), dtype=torch.float32, device=src.device)
        a.norm_table, a.out_pixels = norm_table.data_ptr(), pix.data_ptr()
    if want_u8:
        u8 = torch.empty((T, out_h, out_w, 3), dtype=torch.uint8, device=src.device)
        a.out_u8 = u8.data_ptr()
    ws, need = _workspace(src.device, "am_image_resample_workspace_bytes", T, max(f.n_rows for f in frames), int(out_w), at_least=16)
    a.workspace, a.workspace_bytes = _p(ws), need
    _call(src, None, "am_image_resample", C.byref(a))
    return pix, u8


def image_materialize(src: torch.Tensor, channels: int, frames, frames_dev: torch.Tensor, out_bytes: int,
                      composite: Optional[torch.Tensor] = None, fill: int = 255) -> torch.Tensor:
    """am_image_materialize: the padded (and, for RGBA, composited) frames as flat uint8; frame t is (h + 2 pad_y, w + 2 pad_x, 3) at
    its dst_offset."""
    a = L.AmImageMaterializeArgs()
    _image_src(a, src, channels, composite, fill, frames, frames_dev)
    out = torch.empty((int(out_bytes),), dtype=torch.uint8, device=src.device)
    a.out, a.out_bytes = out.data_ptr(), out.numel()
    _call(src, None, "am_image_materialize", C.byref(a))
    return out


# ---- connected components (csrc/am_components.hip; the contract is the header's) -----------------------------------------------------
def mask_refine(mask: torch.Tensor, min_size: int = 200, threshold: int = -1, return_labels: bool = False, return_stats: bool = False):
    """am_mask_refine: mask (T, H, W) uint8 on the device -> (out_mask uint8 (T, H, W) of 0 / 255, labels int32 (T, H, W) or None,
    stats int32 (T, 4) = [threshold used, foreground pixels, components, components kept] or None), all on the device, nothing read
    back.  `threshold`: -1 = Otsu per frame, 0..255 = that value for every frame.  The argument checks come before the device check,
    so they hold for any tensor."""
    if not isinstance(mask, torch.Tensor):
        raise TypeError(f"mask_refine: expected a torch tensor, got {type(mask).__name__}")
    if mask.dtype != torch.uint8:
        raise TypeError(f"mask_refine: expected a uint8 mask, got {mask.dtype}")
    if mask.dim() != 3 or mask.numel() == 0:
        raise ValueError(f"mask_refine: expected a non-empty (T, H, W) mask, got {tuple(mask.shape)}")
    if not mask.is_contiguous():
        raise ValueError("mask_refine: the mask must be contiguous")
    min_size, threshold = int(min_size), int(threshold)
    if min_size < 0:
        raise ValueError(f"mask_refine: min_size {min_size} is negative")
    if not -1 <= threshold <= 255:
        raise ValueError(f"mask_refine: threshold {threshold} outside -1 .. 255")
    T, H, W = mask.shape
    if H * W >= 2 ** 31 - 1:
        raise ValueError(f"mask_refine: {H} x {W} pixels per frame do not fit a 32-bit label")
    if not mask.is_cuda:
        raise RuntimeError("mask_refine: actionmesh_amd kernels need a device tensor (no CPU path)")
    dev = mask.device
    out = torch.empty_like(mask)
    labels = torch.empty((T, H, W), dtype=torch.int32, device=dev) if return_labels else None
    stats = torch.empty((T, 4), dtype=torch.int32, device=dev) if return_stats else None
    ws, need = _workspace(dev, "am_mask_refine_workspace_bytes", T, H, W)
    a = L.AmMaskRefineArgs()
    a.mask, a.n_frames, a.height, a.width, a.min_size, a.threshold = mask.data_ptr(), T, H, W, min_size, threshold
    a.out_mask, a.out_labels, a.out_stats = out.data_ptr(), _p(labels), _p(stats)
    a.workspace, a.workspace_bytes = _p(ws), need
    _call(mask, None, "am_mask_refine", C.byref(a))
    return out, labels, stats


def graph_components(n_nodes: int, edges: torch.Tensor, return_size: bool = False):
    """am_graph_components: the connected components of an undirected graph of `n_nodes` nodes.  edges (E, 2) int32 on the device
    (self-loops and duplicates allowed, E may be 0).  Returns the int32 label of every node - the smallest node index of its
    component - and with `return_size` also the int32 size of every node's component.  The edge list is validated on the device;
    ONE device-to-host read behind the launch (the flag, which shares the labels' buffer) turns a node index outside [0, n_nodes)
    into a ValueError."""
    if not isinstance(edges, torch.Tensor):
        raise TypeError(f"graph_components: expected a torch tensor of edges, got {type(edges).__name__}")
    if edges.dtype != torch.int32:
        raise TypeError(f"graph_components: expected int32 edges, got {edges.dtype}")
    if edges.dim() != 2 or edges.shape[1] != 2:
        raise ValueError(f"graph_components: expected (E, 2) edges, got {tuple(edges.shape)}")
    if not edges.is_contiguous():
        raise ValueError("graph_components: the edges must be contiguous")
    n = int(n_nodes)
    if not 1 <= n < 2 ** 31 - 1:
        raise ValueError(f"graph_components: n_nodes {n} outside 1 .. 2^31 - 2")
    if not edges.is_cuda:
        raise RuntimeError("graph_components: actionmesh_amd kernels need a device tensor (no CPU path)")
    dev = edges.device
    E = edges.shape[0]
    buf = torch.empty((n + 1,), dtype=torch.int32, device=dev)       # labels, then the flag
    size = torch.empty((n,), dtype=torch.int32, device=dev) if return_size else None
    ws, need = _workspace(dev, "am_graph_components_workspace_bytes", n, E)
    a = L.AmGraphArgs()
    a.n_nodes, a.n_edges, a.edges = n, E, (edges.data_ptr() if E else None)
    a.out_label, a.out_size, a.out_flag = buf.data_ptr(), _p(size), buf.data_ptr() + 4 * n
    a.workspace, a.workspace_bytes = _p(ws), need
    _call(edges, None, "am_graph_components", C.byref(a))
    if bool(buf[n]):
        raise ValueError(f"graph_components: an edge names a node outside [0, {n})")
    label = buf[:n]
    return (label, size) if return_size else label


# ---- anchor-mesh preparation (csrc/am_mesh.hip; the contract is the header's, the tensor interface is mesh_prep.py's) ----------------
_MESH_MAX = (2 ** 31 - 1) // 3
_MESH_FLAGS = {L.MESH_BAD_FACE: "a face names a vertex outside [0, {V})",
               L.MESH_BAD_CSR: "the vertex -> corner CSR does not belong to these faces"}


# What this section, the decimator's and the iso-surface's share: the operand checks and the one path a flag word takes.
def _shaped(what: str, t: torch.Tensor, dtype, shape, dev) -> torch.Tensor:
    """A contiguous tensor of this dtype, shape and device."""
    _need(t, dtype, what)
    if tuple(t.shape) != tuple(shape) or t.device != dev:
        raise ValueError(f"{what}: {tuple(t.shape)} on {t.device}, expected {tuple(shape)} on {dev}")
    return t


def _out(what: str, out: Optional[torch.Tensor], shape, dtype, device) -> torch.Tensor:
    """A fresh contiguous output, or the caller's of the same shape and dtype."""
    return torch.empty(shape, dtype=dtype, device=device) if out is None else _shaped(what, out, dtype, shape, device)


def _positions(what: str, positions: torch.Tensor):
    """Non-empty contiguous (V, 3) fp64 positions.  Returns (V, device)."""
    if not isinstance(positions, torch.Tensor) or positions.dim() != 2 or positions.shape[1] != 3 or positions.shape[0] < 1:
        raise ValueError(f"{what}: expected non-empty (V, 3) positions, got {tuple(getattr(positions, 'shape', ()))}")
    _need(positions, torch.float64, f"{what}: positions")
    return positions.shape[0], positions.device


def _flag_message(table: dict, bits: int, **values) -> str:
    """What the set bits of a flag word say, by the bit -> message table of its entry points."""
    return "; ".join(msg.format(**values) for bit, msg in table.items() if bits & bit)


def _flag_word(what: str, flag: Optional[torch.Tensor], dev) -> Tuple[torch.Tensor, bool]:
    """The flag word of one call: the caller's int32 (1,) tensor - who then reads it, together with whatever else it needs from the
    device - or a fresh one that the wrapper reads itself (`_raise_own_flag`)."""
    if flag is None:
        return torch.empty((1,), dtype=torch.int32, device=dev), True
    _need(flag, torch.int32, f"{what}: flag")
    if flag.numel() != 1 or flag.device != dev:
        raise ValueError(f"{what}: the flag must be one int32 on {dev}")
    return flag, False


def _raise_own_flag(what: str, flag: torch.Tensor, own: bool, table: dict, **values) -> None:
    """Behind the launch, for a flag word the wrapper made itself: ONE device-to-host read, and a set bit is a ValueError."""
    bits = int(flag) if own else 0
    if bits:
        raise ValueError(f"{what}: " + _flag_message(table, bits, **values))


def _mesh_operands(what: str, vertices: torch.Tensor, faces: torch.Tensor, frames: bool):
    """The (vertices, faces) checks the three mesh entry points share; they come before the device check, so they hold for any
    tensor.  Returns (T, V, F, frame stride in elements)."""
    if not isinstance(vertices, torch.Tensor) or not isinstance(faces, torch.Tensor):
        raise TypeError(f"{what}: expected torch tensors")
    if vertices.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{what}: expected float32 or float64 vertices, got {vertices.dtype}")
    if faces.dtype != torch.int32:
        raise TypeError(f"{what}: expected int32 faces, got {faces.dtype}")
    if vertices.dim() not in ((2, 3) if frames else (2,)) or vertices.shape[-1] != 3 or vertices.numel() == 0:
        raise ValueError(f"{what}: expected non-empty {'(V, 3) or (T, V, 3)' if frames else '(V, 3)'} vertices, got {tuple(vertices.shape)}")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{what}: expected (F, 3) faces, got {tuple(faces.shape)}")
    if not faces.is_contiguous():
        raise ValueError(f"{what}: the faces must be contiguous")
    V, F = vertices.shape[-2], faces.shape[0]
    T = vertices.shape[0] if vertices.dim() == 3 else 1
    if V > _MESH_MAX or F > _MESH_MAX or T > 65535:
        raise ValueError(f"{what}: {T} frames of {V} vertices and {F} faces are more than one call covers")
    stride = vertices.stride()
    if stride[-1] != 1 or (V > 1 and stride[-2] != 3) or (vertices.dim() == 3 and T > 1 and stride[0] < 3 * V):
        raise ValueError(f"{what}: a frame's vertices must be contiguous and frames must not overlap (strides {stride})")
    if not vertices.is_cuda or not faces.is_cuda:
        raise RuntimeError(f"{what}: actionmesh_amd kernels need a device tensor (no CPU path)")
    if faces.device != vertices.device:
        raise ValueError(f"{what}: vertices on {vertices.device}, faces on {faces.device}")
    return T, V, F, (stride[0] if vertices.dim() == 3 and T > 1 else 3 * V)


def _topology_tables(what: str, topology, V: int, F: int):
    """The vertex -> corner CSR of a mesh of V vertices and F faces: int32, contiguous, (V + 1) offsets and (3 F) corners."""
    offsets = _need(topology.offsets, torch.int32, f"{what}: topology.offsets")
    corners = _need(topology.corners, torch.int32, f"{what}: topology.corners")
    if offsets.numel() != V + 1 or corners.numel() != 3 * F:
        raise ValueError(f"{what}: the topology is of {offsets.numel() - 1} vertices and {corners.numel() // 3} faces, the mesh has "
                         f"{V} and {F}")
    return offsets, corners


def vertex_normals(vertices: torch.Tensor, faces: torch.Tensor, topology=None, features: bool = False, return_face_normals: bool = False,
                   out: Optional[torch.Tensor] = None, out_face_normals: Optional[torch.Tensor] = None):
    """am_vertex_normals: trimesh's angle-weighted vertex normals followed by the reference's fp32 F.normalize (the contract is the
    header's).  vertices (V, 3) or (T, V, 3), fp32 or fp64, frames that share `faces` (F, 3) int32; a frame stride above 3 V is passed
    as it is (no copy).  `topology`: the vertex -> corner CSR of the faces, an object with int32 device tensors `.offsets` (V + 1)
    and `.corners` (3 F) - a `mesh_topology.MeshTopology`, built here when None; a caller that keeps its faces keeps it too.
    Returns fp32 normals (..., V, 3), or with `features` (..., V, 6) = position rounded to fp32 | normal; with `return_face_normals`
    also the fp64 unit face normals (..., F, 3).  Faces and CSR are validated on the device: ONE device-to-host read behind the
    launch (the flag) turns a vertex index outside [0, V) into a ValueError.  `out` / `out_face_normals`: the caller's buffers."""
    T, V, F, stride = _mesh_operands("vertex_normals", vertices, faces, frames=True)
    if topology is None:
        topology = MeshTopology(faces, V)
    offsets, corners = _topology_tables("vertex_normals", topology, V, F)
    dev = vertices.device
    lead = tuple(vertices.shape[:-2])
    out = _out("vertex_normals: out", out, lead + (V, 6 if features else 3), torch.float32, dev)
    face_normals = None
    if return_face_normals:
        face_normals = _out("vertex_normals: out_face_normals", out_face_normals, lead + (F, 3), torch.float64, dev)
    flag, own = _flag_word("vertex_normals", None, dev)
    ws, need = _workspace(dev, "am_vertex_normals_workspace_bytes", T, F)
    a = L.AmVertexNormalsArgs()
    a.vertices, a.vertices_f64, a.n_frames = vertices.data_ptr(), int(vertices.dtype == torch.float64), T
    a.n_vertices, a.n_faces, a.frame_stride = V, F, stride
    a.faces, a.offsets, a.corners = (faces.data_ptr() if F else None), offsets.data_ptr(), (corners.data_ptr() if F else None)
    a.out_features, a.out_normals = (out.data_ptr(), None) if features else (None, out.data_ptr())
    a.out_face_normals, a.out_flag = _p(face_normals), flag.data_ptr()
    a.workspace, a.workspace_bytes = _p(ws), need
    _call(vertices, None, "am_vertex_normals", C.byref(a))
    _raise_own_flag("vertex_normals", flag, own, _MESH_FLAGS, V=V)
    return (out, face_normals) if return_face_normals else out


def face_areas(vertices: torch.Tensor, faces: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """am_face_areas: the fp64 area (F,) of every face of one frame.  vertices (V, 3) fp32 or fp64, faces (F, 3) int32, F >= 1.
    ONE device-to-host read behind the launch (the flag) turns a vertex index outside [0, V) into a ValueError."""
    _, V, F, _ = _mesh_operands("face_areas", vertices, faces, frames=False)
    if F < 1:
        raise ValueError("face_areas: the mesh has no faces")
    out = _out("face_areas: out", out, (F,), torch.float64, vertices.device)
    flag, own = _flag_word("face_areas", None, vertices.device)
    a = L.AmFaceAreasArgs()
    a.vertices, a.vertices_f64, a.n_vertices, a.n_faces = vertices.data_ptr(), int(vertices.dtype == torch.float64), V, F
    a.faces, a.out_areas, a.out_flag = faces.data_ptr(), out.data_ptr(), flag.data_ptr()
    _call(vertices, None, "am_face_areas", C.byref(a))
    _raise_own_flag("face_areas", flag, own, _MESH_FLAGS, V=V)
    return out


def surface_sample(vertices: torch.Tensor, faces: torch.Tensor, cdf: torch.Tensor, u_face: torch.Tensor, u_bary: torch.Tensor,
                   with_normals: bool = True, out_points: Optional[torch.Tensor] = None, out_face_index: Optional[torch.Tensor] = None,
                   out_normals: Optional[torch.Tensor] = None):
    """am_surface_sample: trimesh.sample.sample_surface with the caller's uniforms (the contract is the header's).  vertices (V, 3)
    fp32 or fp64, faces (F, 3) int32, cdf (F,) fp64 (the prefix sum of the face areas), u_face (n,) and u_bary (n, 2) fp64 in
    [0, 1).  Returns (points (n, 3) fp64, face_index (n,) int32, the unit face normals (n, 3) fp64 or None).  ONE device-to-host
    read behind the launch (the flag) turns a vertex index outside [0, V) in a picked face into a ValueError."""
    _, V, F, _ = _mesh_operands("surface_sample", vertices, faces, frames=False)
    if F < 1:
        raise ValueError("surface_sample: the mesh has no faces")
    _need(cdf, torch.float64, "surface_sample: cdf")
    _need(u_face, torch.float64, "surface_sample: u_face")
    _need(u_bary, torch.float64, "surface_sample: u_bary")
    n = u_face.numel()
    if cdf.numel() != F or n < 1 or n > _MESH_MAX or tuple(u_bary.shape) != (n, 2):
        raise ValueError(f"surface_sample: cdf {tuple(cdf.shape)}, u_face {tuple(u_face.shape)}, u_bary {tuple(u_bary.shape)} "
                         f"do not fit {F} faces and (n,), (n, 2) uniforms")
    dev = vertices.device
    points = _out("surface_sample: out_points", out_points, (n, 3), torch.float64, dev)
    normals = _out("surface_sample: out_normals", out_normals, (n, 3), torch.float64, dev) if with_normals else None
    idx = _out("surface_sample: out_face_index", out_face_index, (n,), torch.int32, dev)
    flag, own = _flag_word("surface_sample", None, dev)
    a = L.AmSurfaceSampleArgs()
    a.vertices, a.vertices_f64, a.n_vertices, a.n_faces, a.n_samples = vertices.data_ptr(), int(vertices.dtype == torch.float64), V, F, n
    a.faces, a.cdf, a.u_face, a.u_bary = faces.data_ptr(), cdf.data_ptr(), u_face.data_ptr(), u_bary.data_ptr()
    a.out_points, a.out_face_index, a.out_normals, a.out_flag = points.data_ptr(), idx.data_ptr(), _p(normals), flag.data_ptr()
    _call(vertices, None, "am_surface_sample", C.byref(a))
    _raise_own_flag("surface_sample", flag, own, _MESH_FLAGS, V=V)
    return points, idx, normals


# ---- mesh decimation (csrc/am_decimate.hip; the contract is the header's, the round loop is mesh_decimate.py's) ----------------------
_DECIMATE_FLAGS = {**_MESH_FLAGS,           # L.DECIMATE_BAD_FACE, L.DECIMATE_BAD_CSR: the same two bits, the same two messages
                   L.DECIMATE_BAD_EDGE: "the edge tables do not belong to these faces",
                   L.DECIMATE_BAD_KEPT: "a kept edge index is outside the edge list"}


def decimate_flag_message(bits: int, V: int) -> str:
    """What the set bits of an am_decimate_* flag word say."""
    return _flag_message(_DECIMATE_FLAGS, bits, V=V)


def _decimate_mesh(what: str, faces: torch.Tensor, topology, V: int, dev=None) -> int:
    """The checks on (faces, CSR) the four entry points share; `dev`: the positions' device, where the call has positions.
    Returns F."""
    if not isinstance(faces, torch.Tensor):
        raise TypeError(f"{what}: expected torch tensors")
    _need(faces, torch.int32, f"{what}: faces")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError(f"{what}: expected non-empty (F, 3) faces, got {tuple(faces.shape)}")
    F = faces.shape[0]
    if not 1 <= V <= _MESH_MAX or F > _MESH_MAX:
        raise ValueError(f"{what}: {V} vertices and {F} faces are outside 1 .. (2^31 - 1) / 3")
    offsets, corners = _topology_tables(what, topology, V, F)
    if offsets.device != faces.device or corners.device != faces.device:
        raise ValueError(f"{what}: the topology is not on {faces.device}")
    if dev is not None and faces.device != dev:
        raise ValueError(f"{what}: positions on {dev}, faces on {faces.device}")
    return F


def _decimate_edge_tables(what: str, a, edges: torch.Tensor, half_edge_to_edge: Optional[torch.Tensor], F: int, dev) -> int:
    """Checks and sets edges (E, 2) and, when given, half_edge_to_edge (3 F).  Returns E."""
    if not isinstance(edges, torch.Tensor) or edges.dim() != 2 or edges.shape[1] != 2 or edges.shape[0] < 1:
        raise ValueError(f"{what}: expected non-empty (E, 2) edges, got {tuple(getattr(edges, 'shape', ()))}")
    E = edges.shape[0]
    _shaped(f"{what}: edges", edges, torch.int32, (E, 2), dev)
    a.n_edges, a.edges = E, edges.data_ptr()
    if half_edge_to_edge is not None:
        a.half_edge_to_edge = _shaped(f"{what}: half_edge_to_edge", half_edge_to_edge, torch.int32, (3 * F,), dev).data_ptr()
    return E


def _decimate_quadrics(what: str, entry: str, a, positions, faces, topology, out, flag, border_operands=None):
    """decimate_quadrics and decimate_border_quadrics: the same operands, checks and output behind two entry points.
    `border_operands(F, dev)` checks and sets what only the border entry takes, in its place: behind the mesh, before the output."""
    V, dev = _positions(what, positions)
    F = _decimate_mesh(what, faces, topology, V, dev)
    if border_operands is not None:
        border_operands(F, dev)
    out = _out(f"{what}: out", out, (V, 10), torch.float64, dev)
    flag, own = _flag_word(what, flag, dev)
    a.positions, a.n_vertices, a.n_faces, a.faces = positions.data_ptr(), V, F, faces.data_ptr()
    a.offsets, a.corners, a.out_quadrics, a.out_flag = topology.offsets.data_ptr(), topology.corners.data_ptr(), out.data_ptr(), flag.data_ptr()
    _call(positions, None, entry, C.byref(a))
    _raise_own_flag(what, flag, own, _DECIMATE_FLAGS, V=V)
    return out


def decimate_quadrics(positions: torch.Tensor, faces: torch.Tensor, topology, out: Optional[torch.Tensor] = None,
                      flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """am_decimate_quadrics: the area-weighted plane quadrics (V, 10) fp64 of every vertex, summed over its faces in the CSR order
    of `topology` (a `mesh_topology.MeshTopology` of `faces`).  positions (V, 3) fp64, faces (F, 3) int32.  Without `flag`, ONE
    device-to-host read behind the launch turns a bad face index or CSR into a ValueError; with the caller's int32 (1,) `flag`
    nothing is read here."""
    return _decimate_quadrics("decimate_quadrics", "am_decimate_quadrics", L.AmDecimateQuadricsArgs(), positions, faces, topology, out, flag)


def _decimate_edges(what: str, entry: str, a, positions, quadrics, faces, topology, edges, half_edge_to_edge, edge_count, out_positions,
                    out_cost, out_key, flag):
    """decimate_edges and decimate_border_edges: the same operands, checks and outputs behind two entry points."""
    V, dev = _positions(what, positions)
    _shaped(f"{what}: quadrics", quadrics, torch.float64, (V, 10), dev)
    F = _decimate_mesh(what, faces, topology, V, dev)
    E = _decimate_edge_tables(what, a, edges, half_edge_to_edge, F, dev)
    a.edge_count = _shaped(f"{what}: edge_count", edge_count, torch.int32, (E,), dev).data_ptr()
    cand = _out(f"{what}: out_positions", out_positions, (E, 3), torch.float64, dev)
    cost = _out(f"{what}: out_cost", out_cost, (E,), torch.float64, dev)
    key = _out(f"{what}: out_key", out_key, (E,), torch.int64, dev)
    flag, own = _flag_word(what, flag, dev)
    a.positions, a.quadrics, a.n_vertices, a.n_faces, a.faces = positions.data_ptr(), quadrics.data_ptr(), V, F, faces.data_ptr()
    a.offsets, a.corners = topology.offsets.data_ptr(), topology.corners.data_ptr()
    a.out_positions, a.out_cost, a.out_key, a.out_flag = cand.data_ptr(), cost.data_ptr(), key.data_ptr(), flag.data_ptr()
    _call(positions, None, entry, C.byref(a))
    _raise_own_flag(what, flag, own, _DECIMATE_FLAGS, V=V)
    return cand, cost, key


def decimate_edges(positions: torch.Tensor, quadrics: torch.Tensor, faces: torch.Tensor, topology, edges: torch.Tensor,
                   half_edge_to_edge: torch.Tensor, edge_count: torch.Tensor, out_positions: Optional[torch.Tensor] = None,
                   out_cost: Optional[torch.Tensor] = None, out_key: Optional[torch.Tensor] = None,
                   flag: Optional[torch.Tensor] = None):
    """am_decimate_edges: for every undirected edge (E, 2) int32 of the live faces, the position a collapse would give the
    surviving vertex (E, 3) fp64, its quadric cost (E,) fp64, and the int64 key (E,) - `_lib.DECIMATE_NO_KEY` where the edge is not a
    candidate (the tests are the header's).  half_edge_to_edge (3 F,) and edge_count (E,) int32.  `flag` as in decimate_quadrics."""
    return _decimate_edges("decimate_edges", "am_decimate_edges", L.AmDecimateEdgesArgs(), positions, quadrics, faces, topology, edges,
                           half_edge_to_edge, edge_count, out_positions, out_cost, out_key, flag)


def decimate_border_quadrics(positions: torch.Tensor, faces: torch.Tensor, topology, half_edge_to_edge: torch.Tensor,
                             edge_count: torch.Tensor, border_weight: float = 1.0, out: Optional[torch.Tensor] = None,
                             flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """am_decimate_border_quadrics: decimate_quadrics plus, for every half-edge whose edge has count 1, one constraint plane through
    the edge and perpendicular to its face, weighted border_weight * |edge|^2 (finite, >= 0), in the header's order.
    half_edge_to_edge (3 F,) and edge_count (E,) int32 are `mesh_topology.EdgeTables`'.  `flag` as in decimate_quadrics."""
    what = "decimate_border_quadrics"
    a = L.AmDecimateBorderQuadricsArgs()

    def border_operands(F, dev):
        weight = float(border_weight)
        if not (math.isfinite(weight) and weight >= 0.0):
            raise ValueError(f"{what}: border_weight {weight} is not finite and >= 0")
        if not isinstance(edge_count, torch.Tensor) or edge_count.dim() != 1 or edge_count.numel() < 1:
            raise ValueError(f"{what}: expected a non-empty (E,) edge_count, got {tuple(getattr(edge_count, 'shape', ()))}")
        E = edge_count.numel()
        a.n_edges, a.border_weight = E, weight
        a.edge_count = _shaped(f"{what}: edge_count", edge_count, torch.int32, (E,), dev).data_ptr()
        a.half_edge_to_edge = _shaped(f"{what}: half_edge_to_edge", half_edge_to_edge, torch.int32, (3 * F,), dev).data_ptr()

    return _decimate_quadrics(what, "am_decimate_border_quadrics", a, positions, faces, topology, out, flag, border_operands)


def decimate_border_edges(positions: torch.Tensor, quadrics: torch.Tensor, faces: torch.Tensor, topology, edges: torch.Tensor,
                          half_edge_to_edge: torch.Tensor, edge_count: torch.Tensor, out_positions: Optional[torch.Tensor] = None,
                          out_cost: Optional[torch.Tensor] = None, out_key: Optional[torch.Tensor] = None,
                          flag: Optional[torch.Tensor] = None):
    """am_decimate_border_edges: decimate_edges with the header's border rule - border vertices move along their border, border
    edges collapse - for the same operands and outputs.  An edge_count that the faces contradict raises the flag's edge bit."""
    return _decimate_edges("decimate_border_edges", "am_decimate_border_edges", L.AmDecimateBorderEdgesArgs(), positions, quadrics, faces,
                           topology, edges, half_edge_to_edge, edge_count, out_positions, out_cost, out_key, flag)


def decimate_select(n_vertices: int, faces: torch.Tensor, topology, edges: torch.Tensor, half_edge_to_edge: torch.Tensor,
                    keys: torch.Tensor, out_m1: Optional[torch.Tensor] = None, out_m2: Optional[torch.Tensor] = None,
                    out_selected: Optional[torch.Tensor] = None, flag: Optional[torch.Tensor] = None):
    """am_decimate_select: the independent set of one round.  Returns (m1 (V,) int64: the smallest key among a vertex's edges, m2
    (V,) int64: the smallest m1 over its closed neighbourhood, selected (E,) uint8: 1 where the edge's key is m2 at both of its ends).
    `flag` as in decimate_quadrics."""
    what = "decimate_select"
    V = int(n_vertices)
    F = _decimate_mesh(what, faces, topology, V)
    dev = faces.device
    a = L.AmDecimateSelectArgs()
    E = _decimate_edge_tables(what, a, edges, half_edge_to_edge, F, dev)
    _shaped(f"{what}: keys", keys, torch.int64, (E,), dev)
    m1 = _out(f"{what}: out_m1", out_m1, (V,), torch.int64, dev)
    m2 = _out(f"{what}: out_m2", out_m2, (V,), torch.int64, dev)
    sel = _out(f"{what}: out_selected", out_selected, (E,), torch.uint8, dev)
    flag, own = _flag_word(what, flag, dev)
    a.n_vertices, a.n_faces, a.faces, a.offsets, a.corners = V, F, faces.data_ptr(), topology.offsets.data_ptr(), topology.corners.data_ptr()
    a.keys, a.out_m1, a.out_m2, a.out_selected, a.out_flag = keys.data_ptr(), m1.data_ptr(), m2.data_ptr(), sel.data_ptr(), flag.data_ptr()
    _call(faces, None, "am_decimate_select", C.byref(a))
    _raise_own_flag(what, flag, own, _DECIMATE_FLAGS, V=V)
    return m1, m2, sel


def decimate_apply(positions: torch.Tensor, quadrics: torch.Tensor, faces: torch.Tensor, topology, edges: torch.Tensor,
                   candidates: torch.Tensor, kept: torch.Tensor, vertex_map: torch.Tensor, out_face_dead: Optional[torch.Tensor] = None,
                   flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """am_decimate_apply: collapse the edges `kept` (K,) int32 - indices into `edges`, a subset of ONE decimate_select's selection -
    IN PLACE: positions[u] = candidates[e], quadrics[u] += quadrics[v], v -> u in the faces of v, vertex_map[v] = u (vertex_map (V,)
    int32).  `topology` is the CSR of the faces BEFORE the call.  Returns face_dead (F,) uint8: 1 on the two faces of every collapsed
    edge, which the caller drops.  `flag` as in decimate_quadrics."""
    what = "decimate_apply"
    V, dev = _positions(what, positions)
    _shaped(f"{what}: quadrics", quadrics, torch.float64, (V, 10), dev)
    F = _decimate_mesh(what, faces, topology, V, dev)
    a = L.AmDecimateApplyArgs()
    E = _decimate_edge_tables(what, a, edges, None, F, dev)
    _shaped(f"{what}: candidates", candidates, torch.float64, (E, 3), dev)
    if not isinstance(kept, torch.Tensor) or kept.dim() != 1 or not 1 <= kept.numel() <= E:
        raise ValueError(f"{what}: expected 1 .. {E} kept edge indices, got {tuple(getattr(kept, 'shape', ()))}")
    K = kept.numel()
    _shaped(f"{what}: kept", kept, torch.int32, (K,), dev)
    _shaped(f"{what}: vertex_map", vertex_map, torch.int32, (V,), dev)
    dead = _out(f"{what}: out_face_dead", out_face_dead, (F,), torch.uint8, dev)
    flag, own = _flag_word(what, flag, dev)
    a.n_vertices, a.n_faces, a.n_kept, a.kept, a.candidates = V, F, K, kept.data_ptr(), candidates.data_ptr()
    a.offsets, a.corners = topology.offsets.data_ptr(), topology.corners.data_ptr()
    a.positions, a.quadrics, a.faces, a.vertex_map = positions.data_ptr(), quadrics.data_ptr(), faces.data_ptr(), vertex_map.data_ptr()
    a.out_face_dead, a.out_flag = dead.data_ptr(), flag.data_ptr()
    _call(positions, None, "am_decimate_apply", C.byref(a))
    _raise_own_flag(what, flag, own, _DECIMATE_FLAGS, V=V)
    return dead


# ---- iso-surface extraction (csrc/am_isosurface.hip; the contract is the header's, the prefix sums and the sizing are isosurface.py's) ----
_GRID_MAX = 2 ** 31 - 1
_ISO_FLAGS = {L.ISO_BAD_VERTEX_OFFSET: "a vertex offset is negative or leads past the vertex count",
              L.ISO_BAD_TRI_OFFSET: "a triangle offset is negative or leads past the triangle count",
              L.ISO_BAD_TABLE: "the crossing masks or triangle counts do not belong to these values"}


def iso_flag_message(bits: int) -> str:
    """What the set bits of an am_iso_* flag word say."""
    return _flag_message(_ISO_FLAGS, bits)


# The grid, count and frame helpers are the dual marching cubes' too.
def _grid(what: str, a, first: torch.Tensor, name: str, dtype, level: Optional[float] = None, others=()):
    """The grid checks the am_iso_* and am_dmc_* entry points share; they come before the device check, so they hold for any tensor.
    `first` (X, Y, Z) of `dtype` sets the grid - the values, where a `level` comes with it -, `others` ((name, tensor, dtype), ...)
    have its shape and device.  Sets nx, ny, nz of `a`, and values and level where given; returns ((nx, ny, nz), device)."""
    if not isinstance(first, torch.Tensor):
        raise TypeError(f"{what}: expected a torch tensor")
    if first.dim() != 3 or min(first.shape) < 2:
        raise ValueError(f"{what}: expected {'' if level is not None else 'an '}(X, Y, Z) {name} with every axis at least 2, got {tuple(first.shape)}")
    if first.numel() > _GRID_MAX:
        raise ValueError(f"{what}: a grid of {tuple(first.shape)} points has more than 2^31 - 1")
    if level is not None:
        level = float(level)
        if level != level or level in (float("inf"), float("-inf")):
            raise ValueError(f"{what}: the level must be finite, got {level}")
    _need(first, dtype, f"{what}: {name}")
    shape, dev = tuple(first.shape), first.device
    for other, t, other_dtype in others:
        _shaped(f"{what}: {other}", t, other_dtype, shape, dev)
    a.nx, a.ny, a.nz = shape
    if level is not None:
        a.values, a.level = first.data_ptr(), level
    return shape, dev


def _grid_counts(what: str, **counts) -> Tuple[int, ...]:
    """n_vertices, or n_vertices and n_triangles (`vertices=`, `triangles=`), as ints inside 1 .. 2^31 - 1."""
    counts = {unit: int(n) for unit, n in counts.items()}
    if not all(1 <= n <= _GRID_MAX for n in counts.values()):
        raise ValueError(f"{what}: " + " and ".join(f"{n} {unit}" for unit, n in counts.items()) + " are outside 1 .. 2^31 - 1")
    return tuple(counts.values())


def _grid_frame(a, origin, spacing) -> None:
    a.origin, a.spacing = ((C.c_double * 3)(*(float(x) for x in three)) for three in (origin, spacing))


def iso_classify(values: torch.Tensor, level: float = 0.0, inside_above: bool = True, out_mask: Optional[torch.Tensor] = None,
                 out_count: Optional[torch.Tensor] = None):
    """am_iso_classify: for every point of the fp32 grid (X, Y, Z) the 7-bit mask of crossing edges that start there, and for every
    cell - at the point of its (0, 0, 0) corner - the number of triangles 0 .. 12 of its six tetrahedra.  Both (X, Y, Z) uint8."""
    what = "iso_classify"
    a = L.AmIsoClassifyArgs()
    shape, dev = _grid(what, a, values, "values", torch.float32, level)
    mask = _out(f"{what}: out_mask", out_mask, shape, torch.uint8, dev)
    count = _out(f"{what}: out_count", out_count, shape, torch.uint8, dev)
    a.inside_above, a.out_mask, a.out_count = int(bool(inside_above)), mask.data_ptr(), count.data_ptr()
    _call(values, None, "am_iso_classify", C.byref(a))
    return mask, count


def iso_vertices(values: torch.Tensor, mask: torch.Tensor, vertex_offset: torch.Tensor, n_vertices: int, origin, spacing,
                 level: float = 0.0, out: Optional[torch.Tensor] = None, flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """am_iso_vertices: the (n_vertices, 3) fp32 positions of the crossing edges, edge (p, m) at vertex_offset[p] + the rank of bit
    m - 1 in mask[p].  mask (X, Y, Z) uint8 from iso_classify, vertex_offset (X, Y, Z) int64: the exclusive prefix sum of the masks'
    popcounts.  origin, spacing: three fp64 numbers each.  `flag` as in decimate_quadrics."""
    what = "iso_vertices"
    a = L.AmIsoVerticesArgs()
    shape, dev = _grid(what, a, values, "values", torch.float32, level, (("mask", mask, torch.uint8), ("vertex_offset", vertex_offset, torch.int64)))
    n_vertices, = _grid_counts(what, vertices=n_vertices)
    out = _out(f"{what}: out", out, (n_vertices, 3), torch.float32, dev)
    flag, own = _flag_word(what, flag, dev)
    _grid_frame(a, origin, spacing)
    a.mask, a.vertex_offset, a.n_vertices, a.out_vertices, a.out_flag = mask.data_ptr(), vertex_offset.data_ptr(), n_vertices, out.data_ptr(), flag.data_ptr()
    _call(values, None, "am_iso_vertices", C.byref(a))
    _raise_own_flag(what, flag, own, _ISO_FLAGS)
    return out


def iso_triangles(values: torch.Tensor, mask: torch.Tensor, count: torch.Tensor, vertex_offset: torch.Tensor, tri_offset: torch.Tensor,
                  n_vertices: int, n_triangles: int, level: float = 0.0, inside_above: bool = True, out: Optional[torch.Tensor] = None,
                  flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """am_iso_triangles: the (n_triangles, 3) int32 faces, the triangles of cell p from row tri_offset[p] on.  mask, count (X, Y, Z)
    uint8 from iso_classify; vertex_offset, tri_offset (X, Y, Z) int64: the exclusive prefix sums of the masks' popcounts and of the
    counts.  `flag` as in decimate_quadrics."""
    what = "iso_triangles"
    a = L.AmIsoTrianglesArgs()
    shape, dev = _grid(what, a, values, "values", torch.float32, level,
                       (("mask", mask, torch.uint8), ("count", count, torch.uint8), ("vertex_offset", vertex_offset, torch.int64),
                        ("tri_offset", tri_offset, torch.int64)))
    n_vertices, n_triangles = _grid_counts(what, vertices=n_vertices, triangles=n_triangles)
    out = _out(f"{what}: out", out, (n_triangles, 3), torch.int32, dev)
    flag, own = _flag_word(what, flag, dev)
    a.inside_above, a.mask, a.count = int(bool(inside_above)), mask.data_ptr(), count.data_ptr()
    a.vertex_offset, a.tri_offset, a.n_vertices, a.n_triangles = vertex_offset.data_ptr(), tri_offset.data_ptr(), n_vertices, n_triangles
    a.out_faces, a.out_flag = out.data_ptr(), flag.data_ptr()
    _call(values, None, "am_iso_triangles", C.byref(a))
    _raise_own_flag(what, flag, own, _ISO_FLAGS)
    return out


# ---- dual marching cubes (csrc/am_dualcubes.hip; the contract is the header's, the prefix sums and the sizing are isosurface.py's) ----
_DMC_FLAGS = {L.DMC_BAD_VERTEX_OFFSET: _ISO_FLAGS[L.ISO_BAD_VERTEX_OFFSET], L.DMC_BAD_TRI_OFFSET: _ISO_FLAGS[L.ISO_BAD_TRI_OFFSET],
              L.DMC_BAD_CODE: "the cell codes or edge masks do not belong to these values"}


def dmc_flag_message(bits: int) -> str:
    """What the set bits of an am_dmc_* flag word say."""
    return _flag_message(_DMC_FLAGS, bits)


def dmc_cells(values: torch.Tensor, level: float = 0.0, inside_above: bool = True, out_config: Optional[torch.Tensor] = None,
              out_double: Optional[torch.Tensor] = None):
    """am_dmc_cells: for every cell of the fp32 grid (X, Y, Z) - at the point of its (0, 0, 0) corner - its configuration, the 8-bit
    inside mask of an active cell (eight finite corners, not all on one side; 0 otherwise), and the 6-bit mask of that
    configuration's double faces.  Both (X, Y, Z) uint8."""
    what = "dmc_cells"
    a = L.AmDmcCellsArgs()
    shape, dev = _grid(what, a, values, "values", torch.float32, level)
    config = _out(f"{what}: out_config", out_config, shape, torch.uint8, dev)
    double = _out(f"{what}: out_double", out_double, shape, torch.uint8, dev)
    a.inside_above, a.out_config, a.out_double = int(bool(inside_above)), config.data_ptr(), double.data_ptr()
    _call(values, None, "am_dmc_cells", C.byref(a))
    return config, double


def dmc_classify(config: torch.Tensor, double: torch.Tensor, out_code: Optional[torch.Tensor] = None,
                 out_count: Optional[torch.Tensor] = None, out_edge_mask: Optional[torch.Tensor] = None):
    """am_dmc_classify: from dmc_cells' two results, per point the cell's code (X, Y, Z) int16 - its configuration, + 256 when its
    double face is double in the neighbour too and so flipped -, its number of patches 0 .. 4 under that code and the 3-bit mask of
    the axis edges from the point that emit a quad (both (X, Y, Z) uint8)."""
    what = "dmc_classify"
    a = L.AmDmcClassifyArgs()
    shape, dev = _grid(what, a, config, "config", torch.uint8, others=(("double", double, torch.uint8),))
    code = _out(f"{what}: out_code", out_code, shape, torch.int16, dev)
    count = _out(f"{what}: out_count", out_count, shape, torch.uint8, dev)
    mask = _out(f"{what}: out_edge_mask", out_edge_mask, shape, torch.uint8, dev)
    a.config, a.double_faces, a.out_code, a.out_count, a.out_edge_mask = (config.data_ptr(), double.data_ptr(), code.data_ptr(),
                                                                          count.data_ptr(), mask.data_ptr())
    _call(config, None, "am_dmc_classify", C.byref(a))
    return code, count, mask


def dmc_vertices(values: torch.Tensor, code: torch.Tensor, vertex_offset: torch.Tensor, n_vertices: int, origin, spacing,
                 level: float = 0.0, inside_above: bool = True, out: Optional[torch.Tensor] = None,
                 flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """am_dmc_vertices: the (n_vertices, 3) fp32 dual vertices, patch q of cell p - the mean of its edges' crossings - at
    vertex_offset[p] + q.  code (X, Y, Z) int16 from dmc_classify, vertex_offset (X, Y, Z) int64: the exclusive prefix sum of its
    patch counts.  origin, spacing: three fp64 numbers each.  `flag` as in decimate_quadrics."""
    what = "dmc_vertices"
    a = L.AmDmcVerticesArgs()
    shape, dev = _grid(what, a, values, "values", torch.float32, level, (("code", code, torch.int16), ("vertex_offset", vertex_offset, torch.int64)))
    n_vertices, = _grid_counts(what, vertices=n_vertices)
    out = _out(f"{what}: out", out, (n_vertices, 3), torch.float32, dev)
    flag, own = _flag_word(what, flag, dev)
    _grid_frame(a, origin, spacing)
    a.inside_above, a.code, a.vertex_offset, a.n_vertices = int(bool(inside_above)), code.data_ptr(), vertex_offset.data_ptr(), n_vertices
    a.out_vertices, a.out_flag = out.data_ptr(), flag.data_ptr()
    _call(values, None, "am_dmc_vertices", C.byref(a))
    _raise_own_flag(what, flag, own, _DMC_FLAGS)
    return out


def dmc_triangles(code: torch.Tensor, edge_mask: torch.Tensor, vertex_offset: torch.Tensor, tri_offset: torch.Tensor,
                  vertices: torch.Tensor, n_vertices: int, n_triangles: int, out: Optional[torch.Tensor] = None,
                  flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """am_dmc_triangles: the (n_triangles, 3) int32 faces, two per emitting edge - its quad over the four cells around it, split
    along the shorter diagonal - from row tri_offset[p] on.  code (X, Y, Z) int16 and edge_mask (X, Y, Z) uint8 from dmc_classify;
    vertex_offset, tri_offset (X, Y, Z) int64: the exclusive prefix sums of the patch counts and of twice the masks' popcounts;
    vertices (n_vertices, 3) fp32 from dmc_vertices.  `flag` as in decimate_quadrics."""
    what = "dmc_triangles"
    a = L.AmDmcTrianglesArgs()
    shape, dev = _grid(what, a, code, "code", torch.int16, others=(("edge_mask", edge_mask, torch.uint8), ("vertex_offset", vertex_offset, torch.int64),
                                                                   ("tri_offset", tri_offset, torch.int64)))
    n_vertices, n_triangles = _grid_counts(what, vertices=n_vertices, triangles=n_triangles)
    _shaped(f"{what}: vertices", vertices, torch.float32, (n_vertices, 3), dev)
    out = _out(f"{what}: out", out, (n_triangles, 3), torch.int32, dev)
    flag, own = _flag_word(what, flag, dev)
    a.code, a.edge_mask, a.vertex_offset, a.tri_offset = code.data_ptr(), edge_mask.data_ptr(), vertex_offset.data_ptr(), tri_offset.data_ptr()
    a.vertices, a.n_vertices, a.n_triangles, a.out_faces, a.out_flag = vertices.data_ptr(), n_vertices, n_triangles, out.data_ptr(), flag.data_ptr()
    _call(code, None, "am_dmc_triangles", C.byref(a))
    _raise_own_flag(what, flag, own, _DMC_FLAGS)
    return out


# ---- exact-fp32 path (csrc/am_f32.hip, am_stage1_f32.hip, am_elementwise.hip; both library builds carry it, `kind` picks which one runs it: same bits) ----
def gemm_f32(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
             gelu: bool = False, out: Optional[torch.Tensor] = None, kind: str = "bf16") -> torch.Tensor:
    """am_gemm_f32: out = act(a @ w.T + bias) + residual, all fp32, fp32 MFMA.  a (M, K), w (N, K) (nn.Linear layout), bias (N,),
    residual / out (M, N); rows may be strided (unit column stride), `residual` may be `out` (in-place residual add).  K % 4 == 0."""
    _need_rows(a, torch.float32, "a"); _need_rows(w, torch.float32, "w")
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError(f"gemm_f32: a is (M, {K}) but w is {tuple(w.shape)}")
    if K % 4:
        raise ValueError(f"gemm_f32: K={K} must be a multiple of 4 (pad the operands)")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    _need_rows(out, torch.float32, "out")
    if tuple(out.shape) != (M, N):
        raise ValueError(f"gemm_f32: out {tuple(out.shape)} != ({M}, {N})")
    if bias is not None:
        _need(bias, torch.float32, "bias")
        if bias.numel() != N:
            raise ValueError(f"gemm_f32: bias has {bias.numel()} elements, N={N}")
    if residual is not None:
        _need_rows(residual, torch.float32, "residual")
        if tuple(residual.shape) != (M, N):
            raise ValueError(f"gemm_f32: residual {tuple(residual.shape)} != ({M}, {N})")
    _call(a, kind, "am_gemm_f32", a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), _p(bias),
            _p(residual), residual.stride(0) if residual is not None else 0, out.data_ptr(), out.stride(0), M, N, K, 1 if gelu else 0)
    return out


def attention_f32(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, sq: int, sk: int, head_dim: int,
                  q_hs: Optional[int] = None, k_hs: Optional[int] = None, v_hs: Optional[int] = None,
                  q_off: int = 0, k_off: int = 0, v_off: int = 0, scale: Optional[float] = None,
                  out: Optional[torch.Tensor] = None, kind: str = "bf16") -> torch.Tensor:
    """am_attention_f32: softmax(Q K^T scale) V in fp32, read in place from projection outputs.  q (nseq * sq, >= ...) and k / v
    (nseq * sk, ...) are 2-D fp32 with unit column stride; head h of row i is columns [x_off + h * x_hs, + head_dim) (x_hs defaults to
    head_dim).  The cross-attention's concatenated [to_k | to_v] output `kv` is k = v = kv, k_hs = v_hs = 2 hd, v_off = hd.
    Returns out (nseq * sq, heads * head_dim) fp32."""
    _need_rows(q, torch.float32, "q"); _need_rows(k, torch.float32, "k"); _need_rows(v, torch.float32, "v")
    if head_dim not in (64, 128):
        raise ValueError(f"attention_f32: head_dim {head_dim} (64 or 128)")
    if sq < 1 or sk < 1 or heads < 1:
        raise ValueError(f"attention_f32: bad shape heads={heads} sq={sq} sk={sk}")
    if q.shape[0] % sq or k.shape[0] % sk or v.shape[0] != k.shape[0] or q.shape[0] // sq != k.shape[0] // sk:
        raise ValueError(f"attention_f32: rows q {q.shape[0]} / k {k.shape[0]} / v {v.shape[0]} do not match sq={sq}, sk={sk}")
    q_hs, k_hs, v_hs = (head_dim if x is None else x for x in (q_hs, k_hs, v_hs))
    for name, t, off, hs in (("q", q, q_off, q_hs), ("k", k, k_off, k_hs), ("v", v, v_off, v_hs)):
        _need_head_columns("attention_f32", name, t, heads, off, hs, head_dim)
    nseq = q.shape[0] // sq
    if out is None:
        out = torch.empty((nseq * sq, heads * head_dim), dtype=torch.float32, device=q.device)
    _need_rows(out, torch.float32, "out")
    if out.shape[0] != nseq * sq or out.shape[1] < heads * head_dim:
        raise ValueError(f"attention_f32: out {tuple(out.shape)} too small for ({nseq * sq}, {heads * head_dim})")
    a = L.AmAttnF32Args()
    a.Q, a.ldq, a.q_off, a.q_hs = q.data_ptr(), q.stride(0), q_off, q_hs
    a.K, a.ldk, a.k_off, a.k_hs = k.data_ptr(), k.stride(0), k_off, k_hs
    a.V, a.ldv, a.v_off, a.v_hs = v.data_ptr(), v.stride(0), v_off, v_hs
    a.O, a.ldo = out.data_ptr(), out.stride(0)
    a.nseq, a.heads, a.sq, a.sk, a.head_dim = nseq, heads, sq, sk, head_dim
    a.scale = scale if scale is not None else head_dim ** -0.5
    _call(q, kind, "am_attention_f32", C.byref(a))
    return out


def layernorm_f32(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float = 1e-5, out: Optional[torch.Tensor] = None,
                  kind: str = "bf16") -> torch.Tensor:
    """am_layernorm_f32: nn.LayerNorm in fp32 over the last axis of x (fp32 in, fp32 out)."""
    _need(x, torch.float32, "x"); _need(w, torch.float32, "w"); _need(b, torch.float32, "b")
    Cdim = x.shape[-1]
    if w.numel() != Cdim or b.numel() != Cdim:
        raise ValueError(f"layernorm_f32: weight / bias of {w.numel()} / {b.numel()} elements for C={Cdim}")
    if out is None:
        out = torch.empty_like(x)
    _need(out, torch.float32, "out")
    if out.data_ptr() == x.data_ptr():
        raise ValueError("layernorm_f32: out may not alias x")
    _call(x, kind, "am_layernorm_f32", x.data_ptr(), out.data_ptr(), w.data_ptr(), b.data_ptr(),
            x.numel() // Cdim, Cdim, eps)
    return out


def head_post_f32(x: torch.Tensor, heads: int, w: torch.Tensor, off: int = 0, head_stride: int = HEAD_DIM, eps: float = 1e-6,
                  rope: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, rows_per_frame: int = 1, kind: str = "bf16") -> torch.Tensor:
    """am_head_post_f32, in place: qk-RMSNorm (gain w (128,), eps) and - with `rope` = (cos, sin), each (frames, 64) fp32 - RoPE with the
    angles of frame row // rows_per_frame, on the 128-wide chunks x[r, off + h * head_stride : + 128] of the packed projection output
    x (rows, >= ...) fp32 (rows may be strided).  One chunk kind per call; the other columns of x are not touched.  Returns x."""
    _need_rows(x, torch.float32, "x"); _need(w, torch.float32, "w")
    if w.numel() != HEAD_DIM:
        raise ValueError(f"head_post_f32: the gain has {w.numel()} elements, head_dim is {HEAD_DIM}")
    _need_head_columns("head_post_f32", "x", x, heads, off, head_stride, HEAD_DIM)
    cos, sin = (None, None) if rope is None else _need_rope_tables("head_post_f32", rope, x.shape[0], rows_per_frame)
    _call(x, kind, "am_head_post_f32", x.data_ptr(), x.stride(0), off, head_stride, x.shape[0], heads, w.data_ptr(), eps,
            _p(cos), _p(sin), 0 if cos is None else cos.shape[0], rows_per_frame)
    return x


def rope_f32(x: torch.Tensor, heads: int, rope: Tuple[torch.Tensor, torch.Tensor], off_a: int = 0, off_b: int = -1,
             head_stride: int = HEAD_DIM, rows_per_frame: int = 1, kind: str = "bf16") -> torch.Tensor:
    """am_rope_f32, in place: RoPE without a qk-norm - `rope` = (cos, sin), each (frames, 64) fp32, the angles of frame
    row // rows_per_frame - on the 128-wide chunks x[r, off_a + h * head_stride : + 128] (q) and, unless off_b < 0, x[r, off_b + h *
    head_stride : + 128] (k) of the packed projection output x (rows, >= ...) fp32 (rows may be strided): both kinds in one launch, the
    bits of the unfused torch fp32 rotation.  The other columns of x are not touched.  Returns x."""
    _need_rows(x, torch.float32, "x")
    for off in (off_a,) if off_b < 0 else (off_a, off_b):
        _need_head_columns("rope_f32", "x", x, heads, off, head_stride, HEAD_DIM)
    cos, sin = _need_rope_tables("rope_f32", rope, x.shape[0], rows_per_frame)
    _call(x, kind, "am_rope_f32", x.data_ptr(), x.stride(0), off_a, off_b, head_stride, x.shape[0], heads, cos.data_ptr(), sin.data_ptr(),
          cos.shape[0], rows_per_frame)
    return x


def flow_step_f32(v: torch.Tensor, latents: torch.Tensor, scales: Sequence[float], dt: float, is_additive: bool,
                  unobserved: Optional[Sequence[bool]], kind: str = "bf16") -> None:
    """am_flow_step_f32, in place: latents (T, N, D) fp32 +- dt * cfg(v) on the unobserved frames, v (n_branches, T, N, D) fp32; every
    operation rounded once to fp32 - the bits of the reference's fp32 expression (guidance.py:95-118, scheduler.py:238-248)."""
    _need(v, torch.float32, "v"); _need(latents, torch.float32, "latents")
    nb, T, N, D = v.shape
    if tuple(latents.shape) != (T, N, D):
        raise ValueError(f"flow_step_f32: latents {tuple(latents.shape)} != {(T, N, D)}")
    if len(scales) < nb - 1 or (unobserved is not None and len(unobserved) != T):
        raise ValueError(f"flow_step_f32: {len(scales)} scales for {nb} branches / a mask that does not cover the {T} frames")
    sc = (C.c_float * max(1, len(scales)))(*[float(s) for s in scales])
    un = None if unobserved is None else (C.c_uint8 * T)(*[1 if u else 0 for u in unobserved])
    _call(v, kind, "am_flow_step_f32", v.data_ptr(), latents.data_ptr(), nb, sc, float(dt), 1 if is_additive else 0, un, T, N, D)


def point_embed_f32(query: torch.Tensor, in_channels: int, extra_channels: int, num_freqs: int, include_pi: bool,
                    ld_out: int = 64, kind: str = "bf16", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`point_embed` without the rounding: query (rows, >= in+extra) fp32, rows may be strided -> fp32 (rows, ld_out)."""
    _need_rows(query, torch.float32, "query")
    if query.dim() != 2 or query.shape[1] < in_channels + extra_channels:
        raise ValueError(f"point_embed_f32: query {tuple(query.shape)} has fewer than {in_channels + extra_channels} channels")
    return _point_embed("point_embed_f32", kind, torch.float32, query, in_channels, extra_channels, num_freqs, include_pi, ld_out, out)


def patchify_f32(pixels: torch.Tensor, patch: int, ld_out: int, kind: str = "bf16", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`patchify` without the rounding: pixels (T, C, H, W) fp32 -> fp32 (T * (H // patch) * (W // patch), ld_out)."""
    _need(pixels, torch.float32, "pixels")
    if pixels.dim() != 4:
        raise ValueError(f"patchify_f32: expected (T, C, H, W), got {tuple(pixels.shape)}")
    return _patchify("patchify_f32", kind, torch.float32, pixels, patch, ld_out, out)


def displacement_f32(logits: torch.Tensor, out_dim: int, out: torch.Tensor, kind: str = "bf16") -> torch.Tensor:
    """out (rows, out_dim) fp32 = 2 sigmoid(-logits[:, :out_dim]) - 1 on fp32 logits (rows may be strided)."""
    _need_rows(logits, torch.float32, "logits"); _need(out, torch.float32, "out")
    if logits.shape[1] < out_dim or out.shape != (logits.shape[0], out_dim):
        raise ValueError(f"displacement_f32: logits {tuple(logits.shape)} / out {tuple(out.shape)} for out_dim={out_dim}")
    return _displacement("displacement_f32", kind, logits, out_dim, out)


def render_normals(vertices: torch.Tensor, faces: torch.Tensor, cameras: Sequence[dict], image_size: int,
                   fragments: bool = False, floats: bool = False) -> dict:
    """am_render_normals: the normal-map preview of an animated mesh.  vertices (T, V, 3) fp32 on the device, faces (F, 3) integer
    (any device: they are moved to the vertices'), cameras: up to 16 dicts with "R" (3, 3), "T" (3,), "focal_length" (fx, fy) and
    "principal_point" (px, py).  Returns {"rgba": uint8 (T, C, S, S, 4)} plus, with `floats`, "mask" (T, C, S, S) and "normal"
    (T, C, S, S, 3), and with `fragments`, "pix_to_face" int32 (T, C, 2S, 2S) and "bary" (T, C, 2S, 2S, 3) - all on the device of
    `vertices`.  The faces are validated on the device: ONE device-to-host read behind the launch (the flag) turns a vertex index
    outside [0, V) into a ValueError."""
    _need(vertices, torch.float32, "vertices")
    if vertices.dim() != 3 or vertices.shape[-1] != 3:
        raise ValueError(f"render_normals: vertices must be (T, V, 3), got {tuple(vertices.shape)}")
    if faces.dim() != 2 or faces.shape[-1] != 3 or faces.dtype.is_floating_point:
        raise ValueError(f"render_normals: faces must be (F, 3) integers, got {tuple(faces.shape)} {faces.dtype}")
    if not 1 <= len(cameras) <= L.RENDER_MAX_CAMERAS:
        raise ValueError(f"render_normals: {len(cameras)} cameras, 1 .. {L.RENDER_MAX_CAMERAS} supported")
    T, V = vertices.shape[0], vertices.shape[1]
    F, Cn, S = faces.shape[0], len(cameras), int(image_size)
    dev = vertices.device
    topology = MeshTopology(faces.detach().to(dev, torch.int32), V)
    out = {"rgba": _out("rgba", None, (T, Cn, S, S, 4), torch.uint8, dev)}
    if floats:
        out["mask"] = _out("mask", None, (T, Cn, S, S), torch.float32, dev)
        out["normal"] = _out("normal", None, (T, Cn, S, S, 3), torch.float32, dev)
    if fragments:
        out["pix_to_face"] = _out("pix_to_face", None, (T, Cn, 2 * S, 2 * S), torch.int32, dev)
        out["bary"] = _out("bary", None, (T, Cn, 2 * S, 2 * S, 3), torch.float32, dev)
    flag, own = _flag_word("render_normals", None, dev)
    a = L.AmRenderArgs()
    a.verts, a.faces = vertices.data_ptr(), topology.faces.data_ptr()
    a.offsets, a.corners, a.out_flag = topology.offsets.data_ptr(), topology.corners.data_ptr(), flag.data_ptr()
    a.n_frames, a.n_verts, a.n_faces, a.n_cameras, a.image_size = T, V, F, Cn, S
    for k, cam in enumerate(cameras):
        c = a.cameras[k]
        R = torch.as_tensor(cam["R"], dtype=torch.float32).reshape(9).tolist()
        Tv = torch.as_tensor(cam["T"], dtype=torch.float32).reshape(3).tolist()
        for i in range(9):
            c.R[i] = R[i]
        for i in range(3):
            c.T[i] = Tv[i]
        c.fx, c.fy = (float(x) for x in cam["focal_length"])
        c.px, c.py = (float(x) for x in cam["principal_point"])
    a.out_rgba = out["rgba"].data_ptr()
    a.out_mask, a.out_normal = _p(out.get("mask")), _p(out.get("normal"))
    a.out_face, a.out_bary = _p(out.get("pix_to_face")), _p(out.get("bary"))
    ws, need = _workspace(dev, "am_render_workspace_bytes", T, V, F, Cn, S, at_least=1)
    _call(vertices, None, "am_render_normals", C.byref(a), ws.data_ptr(), need)
    _raise_own_flag("render_normals", flag, own, _MESH_FLAGS, V=V)
    return out
