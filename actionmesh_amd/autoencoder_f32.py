"""Exact-fp32 Stage II: the forward behind HipAutoencoder(exact_fp32=True).

The reference's fp32 arithmetic (temporal_autoencoder.py:163-269 with autocast off everywhere - what `oracle.autoencoder_forward`
restates), step for step, on the exact-fp32 kernels of the library: am_gemm_f32, am_attention_f32, am_layernorm_f32,
am_point_embed_f32, am_displacement_f32 (csrc/am_f32.hip, am_elementwise.hip) and am_rope_f32 (csrc/am_stage1_f32.hip) - Stage II
rotates q and k without a qk-norm (attention_qk_norm=None, temporal_autoencoder.py:83-92).  Python orchestrates the launches through
ONE backend object (f32_backend.HipF32Backend; the CPU tests substitute torch restatements); torch owns the memory and moves rows,
and does no arithmetic on the device.  Like Stage I's fp32 engine this is the GROUND TRUTH the 16-bit modes are measured against,
not a fast path: nothing is captured in a graph, nothing is sharded.

Layouts, chosen so that no copy is needed:
  * residual stream: frame-major [alpha | N latents], L = N + 1 rows per frame - the 16-bit path's (autoencoder.py).  Attention does
    not care about key order; rows_per_frame = L makes the alpha row of frame f share frame f's angles (temporal_autoencoder.py:216-231).
  * self-attention: [to_q; to_k; to_v] stacked as ONE (3C, C) weight -> the reference's concatenated row viewed as (H, 3 hd)
    (attention_processor.py:105-110): head stride 3 hd, offsets 0 / hd / 2 hd for am_rope_f32 and am_attention_f32 alike.
  * cross-attention: [to_k; to_v] stacked (2C, C), head stride 2 hd (attention_processor.py:111-115).
Once per call: post_quant into the stream, the TimestepEmbedder alpha rows (host sinusoid), the rope tables, the embedded and projected
queries, and the scratch buffers (packed qkv, attention output, ff intermediate), which every block of every target reuses.  Per
target: a fresh copy of the base stream with the T alpha rows written, the self-attention blocks, the cross-attention block on a fresh
copy of the projected queries, am_displacement_f32.  No host read inside the loop.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Optional

import torch

from .denoiser import rope_tables_host

HEAD_DIM = 128
LN_EPS = 1e-5                       # FP32LayerNorm / nn.LayerNorm of the blocks, norm_cross, norm_out


def pack_cross_weights_f32(sd: Dict[str, torch.Tensor], num_layers: int, query_dim: int, query_pad: int, device) -> Dict[str, torch.Tensor]:
    """fp32 device copies of what the reference runs with autocast off: proj_query (K zero-padded to query_pad), the cross-attention
    block with [to_k; to_v] stacked, norm_out, proj_out."""
    p = f"blocks.{num_layers}."
    f32 = lambda t: t.to(device, torch.float32).contiguous()
    pq = torch.zeros((sd["proj_query.weight"].shape[0], query_pad))
    pq[:, :query_dim] = sd["proj_query.weight"]
    w = {"proj_query": f32(pq), "proj_query_b": f32(sd["proj_query.bias"]),
         "q": f32(sd[p + "x_attn.to_q.weight"]),
         "kv": f32(torch.cat([sd[p + "x_attn.to_k.weight"], sd[p + "x_attn.to_v.weight"]], 0)),
         "o": f32(sd[p + "x_attn.to_out.0.weight"]), "o_b": f32(sd[p + "x_attn.to_out.0.bias"]),
         "ff1": f32(sd[p + "ff.net.0.proj.weight"]), "ff1_b": f32(sd[p + "ff.net.0.proj.bias"]),
         "ff2": f32(sd[p + "ff.net.2.weight"]), "ff2_b": f32(sd[p + "ff.net.2.bias"]),
         "proj_out": f32(sd["proj_out.weight"]), "proj_out_b": f32(sd["proj_out.bias"]),
         "norm_out.w": f32(sd["norm_out.weight"]), "norm_out.b": f32(sd["norm_out.bias"])}
    for n, key in (("norm_x_attn", "norm_x_attn"), ("norm_cross", "x_attn.norm_cross"), ("norm_ff", "norm_ff")):
        w[n + ".w"], w[n + ".b"] = f32(sd[p + key + ".weight"]), f32(sd[p + key + ".bias"])
    return w


def pack_self_weights_f32(sd: Dict[str, torch.Tensor], num_layers: int, device) -> Dict[str, torch.Tensor]:
    """fp32 device copies of post_quant and the self-attention blocks, [to_q; to_k; to_v] stacked (3C, C)."""
    f32 = lambda t: t.to(device, torch.float32).contiguous()
    w = {"post_quant": f32(sd["post_quant.weight"]), "post_quant_b": f32(sd["post_quant.bias"])}
    for i in range(num_layers):
        p = f"blocks.{i}."
        w[p + "qkv"] = f32(torch.cat([sd[p + f"s_attn.{n}.weight"] for n in ("to_q", "to_k", "to_v")], 0))
        w[p + "o"], w[p + "o_b"] = f32(sd[p + "s_attn.to_out.0.weight"]), f32(sd[p + "s_attn.to_out.0.bias"])
        w[p + "ff1"], w[p + "ff1_b"] = f32(sd[p + "ff.net.0.proj.weight"]), f32(sd[p + "ff.net.0.proj.bias"])
        w[p + "ff2"], w[p + "ff2_b"] = f32(sd[p + "ff.net.2.weight"]), f32(sd[p + "ff.net.2.bias"])
        for n in ("norm_s_attn", "norm_ff"):
            w[p + n + ".w"], w[p + n + ".b"] = f32(sd[p + n + ".weight"]), f32(sd[p + n + ".bias"])
    return w


def cross_logits(be, w: Dict[str, torch.Tensor], kv32: torch.Tensor, qh32: torch.Tensor, heads: int, V: int, S: int) -> torch.Tensor:
    """blocks[-1](queries, encoder_hidden_states=kv_cache) -> norm_out -> proj_out, all fp32 (temporal_autoencoder.py:152-161).  kv32
    (B*S, C): the finished residual stream (any key order per batch entry); qh32 (B*V, C): proj_query's output, used as the block's
    residual stream (modified in place).  Returns (B*V, out_dim) logits BEFORE the reference's * -1."""
    hd = HEAD_DIM
    e = be.layernorm(kv32, w["norm_cross.w"], w["norm_cross.b"], LN_EPS)          # nn.LayerNorm, eps 1e-5
    kv = be.gemm(e, w["kv"])                                                      # (B*S, 2C) = [to_k | to_v]
    del e
    z = be.layernorm(qh32, w["norm_x_attn.w"], w["norm_x_attn.b"], LN_EPS)
    q = be.gemm(z, w["q"])
    # attention_processor.py:111-115: head h of the concatenated projection is columns h*2hd (K) and h*2hd + hd (V)
    a = be.attention(q, kv, kv, heads, V, S, hd, 2 * hd, 2 * hd, 0, 0, hd)
    del kv, q
    be.gemm(a, w["o"], bias=w["o_b"], residual=qh32, out=qh32)
    z = be.layernorm(qh32, w["norm_ff.w"], w["norm_ff.b"], LN_EPS, out=z)
    f = be.gemm(z, w["ff1"], bias=w["ff1_b"], gelu=True)
    be.gemm(f, w["ff2"], bias=w["ff2_b"], residual=qh32, out=qh32)
    del f
    z = be.layernorm(qh32, w["norm_out.w"], w["norm_out.b"], LN_EPS, out=z)
    return be.gemm(z, w["proj_out"], bias=w["proj_out_b"])


def alpha_embedding_host(width: int, source_alpha: torch.Tensor, target_alphas: torch.Tensor) -> torch.Tensor:
    """TimestepEmbedder(source, target) = [cos | sin](source) | [cos | sin](target), width / 4 frequencies each
    (temporal_autoencoder.py:232-235, embeddings.py:55-130), in fp32 on the host -> (B, T_out, width)."""
    half = width // 4
    freqs = torch.exp(-math.log(10_000) * torch.arange(half, dtype=torch.float32) / half)
    src = source_alpha.detach().float().cpu()[:, None].expand_as(target_alphas)
    emb = []
    for t in (src, target_alphas.detach().float().cpu()):
        arg = t[..., None] * freqs
        emb += [torch.cos(arg), torch.sin(arg)]
    return torch.cat(emb, -1)


def forward_f32(be, ws: Dict[str, torch.Tensor], wx: Dict[str, torch.Tensor], model, latent: torch.Tensor, framestep: torch.Tensor,
                source_alpha: torch.Tensor, target_alphas: torch.Tensor, query: torch.Tensor,
                step_callback: Optional[Callable[[int, int], None]] = None) -> torch.Tensor:
    """temporal_autoencoder.py:163-269 in fp32 through the backend `be`.  ws / wx: pack_self_weights_f32 / pack_cross_weights_f32 on
    the device of the forward; `model`: the HipAutoencoder (its fields only).  latent (B, T, N, D), framestep (B, T), source_alpha
    (B,), target_alphas (B, T_out), query (B, V, in + extra) -> displacement (B, T_out, V, out_dim) fp32."""
    dev, C, H, hd, NL = model.device, model.width, model.heads, HEAD_DIM, model.num_layers
    B, T, N, D = latent.shape
    T_out, V, L = target_alphas.shape[1], query.shape[1], N + 1
    S, rows = T * L, B * T * L
    f32 = dict(dtype=torch.float32, device=dev)
    # once per call: post_quant into the frame-major stream (rows f L + 1 + n; row f L is the alpha token)
    base = torch.zeros((rows, C), **f32)
    lat = latent.to(dev, torch.float32).reshape(B * T * N, D).contiguous()
    base.view(B * T, L, C)[:, 1:] = be.gemm(lat, ws["post_quant"], bias=ws["post_quant_b"]).view(B * T, N, C)
    rope = tuple(t.to(dev) for t in rope_tables_host(framestep))                   # scale_timestep(center) (:198-209): (B*T, 64)
    alpha = alpha_embedding_host(C, source_alpha, target_alphas).to(dev)           # (B, T_out, C)
    q32 = query.to(dev, torch.float32).reshape(B * V, -1).contiguous()
    qe = be.point_embed(q32, model.in_channels, model.in_extra_channels, model.embed_frequency, model.embed_include_pi, model.query_pad)
    qh0 = be.gemm(qe, wx["proj_query"], bias=wx["proj_query_b"])                   # (:240-243)
    del qe, lat
    z, qkv = torch.empty((rows, C), **f32), torch.empty((rows, 3 * C), **f32)
    a, u = torch.empty((rows, C), **f32), torch.empty((rows, ws["blocks.0.ff1"].shape[0]), **f32)
    out = torch.empty((B, T_out, V, model.out_dim), **f32)
    for i in range(T_out):
        if step_callback is not None:
            step_callback(i + 1, T_out)
        h = base.clone()
        h.view(B, T, L, C)[:, :, 0] = alpha[:, i][:, None]                          # (:254), the same alpha token in every frame
        for li in range(NL):                                                       # block.py:137-152, attention_processor.py:92-147
            p = f"blocks.{li}."
            be.layernorm(h, ws[p + "norm_s_attn.w"], ws[p + "norm_s_attn.b"], LN_EPS, out=z)
            be.gemm(z, ws[p + "qkv"], out=qkv)
            be.rope(qkv, H, rope, 0, hd, 3 * hd, L)
            be.attention(qkv, qkv, qkv, H, S, S, 3 * hd, 3 * hd, 3 * hd, 0, hd, 2 * hd, out=a)
            be.gemm(a, ws[p + "o"], bias=ws[p + "o_b"], residual=h, out=h)
            be.layernorm(h, ws[p + "norm_ff.w"], ws[p + "norm_ff.b"], LN_EPS, out=z)
            be.gemm(z, ws[p + "ff1"], bias=ws[p + "ff1_b"], gelu=True, out=u)
            be.gemm(u, ws[p + "ff2"], bias=ws[p + "ff2_b"], residual=h, out=h)
        lg = cross_logits(be, wx, h, qh0.clone(), H, V, S)
        for b in range(B):
            be.displacement(lg[b * V:(b + 1) * V], model.out_dim, out[b, i])
        del h, lg
    return out
