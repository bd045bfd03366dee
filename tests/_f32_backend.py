"""The torch-CPU restatement of `actionmesh_amd.f32_backend.HipF32Backend`: its methods - and ops.flow_step for an fp32 velocity, the
sampler's fifth kernel of Stage I - as plain torch fp32 statements on CPU tensors, written from the contracts in
include/actionmesh_amd.h (same in-place and aliasing behaviour, the same count names), so that the orchestration of the exact-fp32
forwards (Stage I, Stage II, the image encoder) runs without a device.  tests/_stage1_fp32.py, tests/_stage2_fp32.py and
tests/test_encoder_fp32_cpu.py share it."""
import torch
import torch.nn.functional as F

HD = 128          # the chunk width of am_head_post_f32 and am_rope_f32


def _out(y, out):
    if out is None:
        return y
    out.copy_(y)
    return out


class TorchBackend:
    def __init__(self):
        self.calls = {}

    def _count(self, name):
        self.calls[name] = self.calls.get(name, 0) + 1

    def gemm(self, a, w, bias=None, residual=None, gelu=False, out=None):
        self._count("am_gemm_f32")
        y = F.linear(a, w, bias)
        if gelu:
            y = F.gelu(y, approximate="none")
        if residual is not None:
            y = y + residual
        return _out(y, out)

    def layernorm(self, x, w, b, eps, out=None):
        self._count("am_layernorm_f32")
        assert out is None or out.data_ptr() != x.data_ptr()
        return _out(F.layer_norm(x, (x.shape[-1],), w, b, eps), out)

    @staticmethod
    def _rotate(c, rope, rows_per_frame):
        """out = x cos + rot(x) sin on (rows, 128) chunks, the angles of frame row // rows_per_frame."""
        rows = c.shape[0]
        frame = torch.arange(rows) // rows_per_frame
        cs, sn = (t[frame].repeat_interleave(2, dim=1) for t in rope)
        xr, xi = c.reshape(rows, HD // 2, 2).unbind(-1)
        return c * cs + torch.stack([-xi, xr], dim=-1).flatten(1) * sn

    def head_post(self, x, heads, w, off, head_stride, eps, rope=None, rows_per_frame=1):
        self._count("am_head_post_f32")
        for h in range(heads):
            c = x[:, off + h * head_stride: off + h * head_stride + HD]
            y = c * torch.rsqrt(c.pow(2).mean(-1, keepdim=True) + eps) * w
            c.copy_(y if rope is None else self._rotate(y, rope, rows_per_frame))
        return x

    def rope(self, x, heads, rope, off_a, off_b, head_stride, rows_per_frame):
        self._count("am_rope_f32")
        for off in (off_a,) if off_b < 0 else (off_a, off_b):
            for h in range(heads):
                c = x[:, off + h * head_stride: off + h * head_stride + HD]
                c.copy_(self._rotate(c, rope, rows_per_frame))
        return x

    def attention(self, q, k, v, heads, sq, sk, q_hs, k_hs, v_hs, q_off, k_off, v_off, out=None, head_dim=HD):
        self._count("am_attention_f32")
        nseq, D = q.shape[0] // sq, head_dim

        def split(t, s, off, hs):
            return torch.stack([t[:, off + h * hs: off + h * hs + D] for h in range(heads)], 0).reshape(heads, nseq, s, D).transpose(0, 1)
        o = F.scaled_dot_product_attention(split(q, sq, q_off, q_hs), split(k, sk, k_off, k_hs), split(v, sk, v_off, v_hs))
        return _out(o.transpose(1, 2).reshape(nseq * sq, heads * D).contiguous(), out)

    def point_embed(self, query, in_channels, extra_channels, num_freqs, include_pi, ld_out):
        self._count("am_point_embed_f32")
        x = query[:, :in_channels]
        freqs = 2.0 ** torch.arange(num_freqs, dtype=torch.float32)
        if include_pi:
            freqs = freqs * torch.pi
        e = (x[..., None] * freqs).reshape(x.shape[0], -1)
        cat = torch.cat([x, e.sin(), e.cos(), query[:, in_channels:in_channels + extra_channels]], -1)
        out = torch.zeros((query.shape[0], ld_out))
        out[:, :cat.shape[1]] = cat
        return out

    def patchify(self, pixels, patch, ld_out):
        self._count("am_patchify_f32")
        cols = F.unfold(pixels, patch, stride=patch).transpose(1, 2).reshape(-1, pixels.shape[1] * patch * patch)
        out = torch.zeros((cols.shape[0], ld_out))
        out[:, :cols.shape[1]] = cols
        return out

    def displacement(self, logits, out_dim, out):
        self._count("am_displacement_f32")
        out.copy_(2 * torch.sigmoid(-logits[:, :out_dim]) - 1.0)
        return out

    def flow_step(self, v, latents, scales, dt, is_additive, unobserved):
        self._count("am_flow_step_f32")
        assert v.dtype == torch.float32 and latents.dtype == torch.float32
        out = v[0]
        for i in range(v.shape[0] - 1):
            out = out + float(scales[i]) * (v[i + 1] - v[i])
        step = torch.tensor(dt, dtype=torch.float32) * out
        flow = latents + step if is_additive else latents - step
        sel = torch.ones(latents.shape[0], dtype=torch.bool) if unobserved is None else torch.tensor([bool(u) for u in unobserved])
        latents[sel] = flow[sel]
