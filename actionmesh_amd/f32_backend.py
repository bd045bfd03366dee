"""The one door to the kernels of the exact-fp32 path.  Stage I (denoiser_f32.F32Engine), the exact Stage II (autoencoder_f32), the cross_fp32
mode of HipAutoencoder and HipImageEncoder(dtype="float32") all launch through an object with these methods, so that their orchestration
runs on restatements of them too (the CPU tests substitute torch ones).  am_flow_step_f32 is the sampler's, not a model's: ops.flow_step."""
from collections import Counter

from . import ops


class HipF32Backend:
    def __init__(self, kind: str = "bf16"):
        self.kind = kind             # which build of the library runs the fp32 entry points (the same bits from both)
        self.calls = Counter()       # launches per C entry point: what really ran

    def gemm(self, a, w, bias=None, residual=None, gelu=False, out=None):
        self.calls["am_gemm_f32"] += 1
        return ops.gemm_f32(a, w, bias=bias, residual=residual, gelu=gelu, out=out, kind=self.kind)

    def layernorm(self, x, w, b, eps, out=None):
        self.calls["am_layernorm_f32"] += 1
        return ops.layernorm_f32(x, w, b, eps=eps, out=out, kind=self.kind)

    def head_post(self, x, heads, w, off, head_stride, eps, rope=None, rows_per_frame=1):
        self.calls["am_head_post_f32"] += 1
        return ops.head_post_f32(x, heads, w, off=off, head_stride=head_stride, eps=eps, rope=rope, rows_per_frame=rows_per_frame,
                                 kind=self.kind)

    def attention(self, q, k, v, heads, sq, sk, q_hs, k_hs, v_hs, q_off, k_off, v_off, out=None, head_dim=ops.HEAD_DIM):
        self.calls["am_attention_f32"] += 1
        return ops.attention_f32(q, k, v, heads, sq, sk, head_dim, q_hs=q_hs, k_hs=k_hs, v_hs=v_hs, q_off=q_off, k_off=k_off,
                                 v_off=v_off, out=out, kind=self.kind)

    def rope(self, x, heads, rope, off_a, off_b, head_stride, rows_per_frame):
        self.calls["am_rope_f32"] += 1
        return ops.rope_f32(x, heads, rope, off_a=off_a, off_b=off_b, head_stride=head_stride, rows_per_frame=rows_per_frame,
                            kind=self.kind)

    def point_embed(self, query, in_channels, extra_channels, num_freqs, include_pi, ld_out):
        self.calls["am_point_embed_f32"] += 1
        return ops.point_embed_f32(query, in_channels, extra_channels, num_freqs, include_pi, ld_out, kind=self.kind)

    def patchify(self, pixels, patch, ld_out):
        self.calls["am_patchify_f32"] += 1
        return ops.patchify_f32(pixels, patch, ld_out, kind=self.kind)

    def displacement(self, logits, out_dim, out):
        self.calls["am_displacement_f32"] += 1
        return ops.displacement_f32(logits, out_dim, out, kind=self.kind)
