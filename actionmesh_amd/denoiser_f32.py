"""Exact-fp32 Stage I: the engine behind HipDenoiser(dtype="float32").

The forward is the reference's fp32 arithmetic (temporal_denoiser.py:151-249 with autocast off - what `oracle.denoiser_forward(...,
"fp32")` restates), step for step, on the exact-fp32 kernels of the library: am_gemm_f32, am_attention_f32, am_layernorm_f32 (csrc/
am_f32.hip) and am_head_post_f32 (csrc/am_stage1_f32.hip); the sampler's CFG + Euler step is am_flow_step_f32.  Python orchestrates
the launches through ONE backend object (f32_backend.HipF32Backend; the CPU tests substitute torch restatements); torch owns the memory and moves rows (the
time token's placement, the final [:, -N:] slice), and does no arithmetic on the device.  This engine is the GROUND TRUTH the 16-bit
and fp8 paths are measured against, not a fast path: every operation is computed (the exact-shortcut hints of the 16-bit engine are
accepted and ignored), nothing is captured in a graph, nothing is sharded.

How the existing kernels fit the reference's layouts without a copy:
  * self-attention: [to_q; to_k; to_v] stacked as ONE (3C, C) weight -> one GEMM whose output row is the reference's concatenated
    q | k | v row (attention_processor.py:106-110), which it views as (H, 3 hd): head h has q at column 3 hd h, k at 3 hd h + hd, v at
    3 hd h + 2 hd - offsets 0 / hd / 2 hd with head stride 3 hd, for am_head_post_f32 and am_attention_f32 alike.  Inflated layers:
    B sequences of T L tokens; the others: B T sequences of L tokens.
  * cross-attention: [to_k; to_v] stacked (2C, Dc), head stride 2 hd (attention_processor.py:111-115); the window's K / V - norm_k
    applied - are computed once per bound window (set_context) and kept in fp32.
  * linear_skip on cat(skip, h): two GEMMs on the two column halves of the (C, 2C) weight (ldw = 2C), the second adding into the
    first's output (residual aliasing the output); the concatenated activation is never materialised.
  * time token: the sinusoid on the host in fp32 (t_bt is host data), the two time_proj linears on am_gemm_f32 (erf-GELU fused).
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import torch

from .f32_backend import HipF32Backend

HEAD_DIM = 128
LN_EPS, RMS_EPS = 1e-5, 1e-6        # FP32LayerNorm / nn.LayerNorm (block.py:64,83,98,107); RMSNorm(dim_head, eps=1e-6) (block.py:49,72,91)


def timestep_sinusoid_host(t_bt: Sequence[float], dim: int) -> torch.Tensor:
    """diffusers Timesteps(dim, flip_sin_to_cos=False, downscale_freq_shift=0) (temporal_denoiser.py:57-61, 213) in fp32 on the host:
    [sin(t f_i) | cos(t f_i)], f_i = exp(-ln(1e4) i / half) - the statements of the reference, so the same fp32 values."""
    half = dim // 2
    exponent = -math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half
    emb = torch.tensor(list(t_bt), dtype=torch.float32)[:, None] * torch.exp(exponent)[None, :]
    return torch.cat([torch.sin(emb), torch.cos(emb)], dim=-1)


def pack_weights_f32(sd: Dict[str, torch.Tensor], hp: Dict) -> Dict[str, torch.Tensor]:
    """Reference state dict -> the fp32 operands of the engine (CPU): the stacked projections, everything else as it is."""
    f = lambda k: sd[k].detach().to("cpu", torch.float32).contiguous()
    w = {k: f(k) for k in sd if ".s_attn.to_" not in k or ".to_out." in k}
    for i in range(hp["num_layers"]):
        p = f"blocks.{i}."
        w[p + "s_attn.qkv.weight"] = torch.cat([f(p + f"s_attn.to_{n}.weight") for n in "qkv"], dim=0).contiguous()
        w[p + "x_attn.kv.weight"] = torch.cat([w.pop(p + f"x_attn.to_{n}.weight") for n in "kv"], dim=0).contiguous()
    return w


class F32Engine:
    """What HipDenoiser uses of HipEngine - fits, set_context, forward(x, t_bt), close, device, kind - in exact fp32.  One device, one
    process; the buffers of a forward are torch allocations of that forward, so every shape fits."""

    kind = "f32"
    world, rank = 1, 0

    def __init__(self, hp: Dict, state_dict: Dict[str, torch.Tensor], device: torch.device, backend=None):
        self.device = torch.device(device)
        if backend is None:
            if self.device.type != "cuda":
                raise RuntimeError("F32Engine needs a ROCm device (torch device type 'cuda'); there is no CPU path")
            backend = HipF32Backend()
        self.backend = backend
        self.hp = dict(hp)
        self.C, self.H, self.NL = hp["width"], hp["num_attention_heads"], hp["num_layers"]
        if self.C != self.H * HEAD_DIM:
            raise ValueError("F32Engine supports head_dim 128 only (width = heads * 128), as the reference ships")
        self.inflated = set(hp["inflated_layers"])
        missing = [k for k in ("proj_in.weight", "norm_out.weight", f"blocks.{self.NL - 1}.ff.net.2.weight") if k not in state_dict]
        if missing:
            raise RuntimeError(f"F32Engine: reference state-dict keys were not provided: {missing}")
        self.w = {k: v.to(self.device) for k, v in pack_weights_f32(state_dict, hp).items()}
        self._kv: Optional[List[torch.Tensor]] = None
        self._rope = None
        self._shape = None

    def close(self, collective: bool = True) -> None:
        self.w, self._kv, self._rope = {}, None, None

    def fits(self, B: int, T: int, N: int, S: int) -> bool:
        return True

    def entry_counts(self) -> Dict[str, int]:
        """Launches per C entry point of this engine so far (HipF32Backend.calls)."""
        return dict(self.backend.calls)

    def has_skip(self, layer: int) -> bool:
        return layer > self.NL // 2                      # temporal_denoiser.py:92

    def set_context(self, ctx_local: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                    ctx_zero: Optional[Sequence[bool]] = None, shared_prefix: bool = False) -> None:
        """ctx_local (B, T, S, Dc) fp32; cos / sin (B*T, 64) fp32 host (rope_tables_host).  The cross-attention K / V of every layer for
        this window: [to_k | to_v](context), norm_k on the K chunks (attention_processor.py:102-103, 111-115, 122-124).  `ctx_zero`
        and `shared_prefix` are the 16-bit engine's exact shortcuts: accepted and ignored, everything is computed."""
        B, T, S, Dc = ctx_local.shape
        be, w, hd = self.backend, self.w, HEAD_DIM
        ctx = ctx_local.to(self.device, torch.float32).reshape(B * T * S, Dc).contiguous()
        assert cos.shape == (B * T, hd // 2) and sin.shape == cos.shape
        self._rope = (cos.to(self.device, torch.float32).contiguous(), sin.to(self.device, torch.float32).contiguous())
        self._kv = []
        for i in range(self.NL):
            p = f"blocks.{i}.x_attn."
            kv = be.gemm(ctx, w[p + "kv.weight"])                                              # (B*T*S, 2C): head h = [k | v] at 2 hd h
            be.head_post(kv, self.H, w[p + "norm_k.weight"], 0, 2 * hd, RMS_EPS)
            self._kv.append(kv)
        self._shape = (B, T, S)

    def forward(self, x_local: torch.Tensor, t_bt_local: List[float]) -> torch.Tensor:
        """x (B, T, N, Din), t_bt the masked per-(b t) diffusion times -> velocity (B, T, N, Din) float32."""
        if self._kv is None:
            raise RuntimeError("F32Engine: set_context() must precede forward()")
        B, T, N, Din = x_local.shape
        if (B, T) != self._shape[:2]:
            raise RuntimeError(f"F32Engine: forward of batch {(B, T)} against a window bound for {self._shape[:2]}")
        be, w, C, H, hd = self.backend, self.w, self.C, self.H, HEAD_DIM
        S, BT, Lt = self._shape[2], B * T, N + 1
        rows = BT * Lt
        x = x_local.to(self.device, torch.float32).reshape(BT * N, Din).contiguous()
        # temporal_denoiser.py:205-217: h = [time token | proj_in(x)] per frame
        h = torch.empty((rows, C), dtype=torch.float32, device=self.device)
        h3 = h.view(BT, Lt, C)
        h3[:, 1:] = be.gemm(x, w["proj_in.weight"], bias=w["proj_in.bias"]).view(BT, N, C)
        e = timestep_sinusoid_host(t_bt_local, C).to(self.device)
        e = be.gemm(e, w["time_proj.linear_1.weight"], bias=w["time_proj.linear_1.bias"], gelu=True)
        h3[:, 0] = be.gemm(e, w["time_proj.linear_2.weight"], bias=w["time_proj.linear_2.bias"])
        z = torch.empty_like(h)
        skips: List[torch.Tensor] = []
        for i in range(self.NL):                                                               # temporal_denoiser.py:222-236
            p = f"blocks.{i}."
            if self.has_skip(i):                                                               # block.py:131-133
                ws = w[p + "linear_skip.weight"]                                               # (C, 2C): columns [skip | h]
                cat = be.gemm(skips.pop(), ws[:, :C], bias=w[p + "linear_skip.bias"])
                be.gemm(h, ws[:, C:], residual=cat, out=cat)
                be.layernorm(cat, w[p + "norm_skip.weight"], w[p + "norm_skip.bias"], LN_EPS, out=h)
                del cat
            # self-attention (block.py:137-142, attention_processor.py:92-147)
            be.layernorm(h, w[p + "norm_s_attn.weight"], w[p + "norm_s_attn.bias"], LN_EPS, out=z)
            qkv = be.gemm(z, w[p + "s_attn.qkv.weight"])
            be.head_post(qkv, H, w[p + "s_attn.norm_q.weight"], 0, 3 * hd, RMS_EPS, rope=self._rope, rows_per_frame=Lt)
            be.head_post(qkv, H, w[p + "s_attn.norm_k.weight"], hd, 3 * hd, RMS_EPS, rope=self._rope, rows_per_frame=Lt)
            s = T * Lt if i in self.inflated else Lt
            a = be.attention(qkv, qkv, qkv, H, s, s, 3 * hd, 3 * hd, 3 * hd, 0, hd, 2 * hd)
            del qkv
            be.gemm(a, w[p + "s_attn.to_out.0.weight"], bias=w[p + "s_attn.to_out.0.bias"], residual=h, out=h)
            # cross-attention against the window's K / V (block.py:146-149)
            be.layernorm(h, w[p + "norm_x_attn.weight"], w[p + "norm_x_attn.bias"], LN_EPS, out=z)
            q = be.gemm(z, w[p + "x_attn.to_q.weight"])
            be.head_post(q, H, w[p + "x_attn.norm_q.weight"], 0, hd, RMS_EPS)
            kv = self._kv[i]
            a = be.attention(q, kv, kv, H, Lt, S, hd, 2 * hd, 2 * hd, 0, 0, hd)
            del q
            be.gemm(a, w[p + "x_attn.to_out.0.weight"], bias=w[p + "x_attn.to_out.0.bias"], residual=h, out=h)
            # feed-forward (block.py:99-104, 152)
            be.layernorm(h, w[p + "norm_ff.weight"], w[p + "norm_ff.bias"], LN_EPS, out=z)
            u = be.gemm(z, w[p + "ff.net.0.proj.weight"], bias=w[p + "ff.net.0.proj.bias"], gelu=True)
            be.gemm(u, w[p + "ff.net.2.weight"], bias=w[p + "ff.net.2.bias"], residual=h, out=h)
            del u, a
            if i < self.NL // 2:
                skips.append(h.clone())                                                        # h is updated in place from here on
        # temporal_denoiser.py:239-247: norm_out, drop the time token, proj_out
        be.layernorm(h, w["norm_out.weight"], w["norm_out.bias"], LN_EPS, out=z)
        tokens = z.view(BT, Lt, C)[:, -N:].reshape(BT * N, C)
        return be.gemm(tokens, w["proj_out.weight"], bias=w["proj_out.bias"]).view(B, T, N, Din)
