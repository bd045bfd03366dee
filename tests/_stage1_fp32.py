"""What tests/test_stage1_fp32_cpu.py and tests/test_stage1_fp32_gpu.py share: the tiny fixtures' cases, torch-CPU restatements of the five
kernels - the four of the forward behind the interface of `actionmesh_amd.denoiser_f32.HipF32Backend`, and the sampler's CFG + Euler
step - so that the orchestration of HipDenoiser(dtype="float32") runs without a device, and the assertions both files make on `tiny_inflated` / `tiny_mixed` - on the restatements in one, on the kernels in
the other.

The bound throughout is rel-L2 <= 2e-5 against the fp32 values of the reference's own modules (tests/golden/tiny_*.npz): the statement
tests/test_fp32_path_gpu.py makes for the 24-layer fp32 encoder against an independent fp32 implementation."""
import os

import numpy as np
import torch
import torch.nn.functional as F

BOUND = 2e-5
HD = 128
CASES = {
    "tiny_inflated": dict(in_channels=64, num_layers=5, num_attention_heads=2, width=256,
                          mlp_ratio=4.0, cross_attention_dim=64, inflated_layers=(0, 1, 2, 3, 4)),
    "tiny_mixed": dict(in_channels=64, num_layers=5, num_attention_heads=2, width=256,
                       mlp_ratio=4.0, cross_attention_dim=64, inflated_layers=(0, 1, 3, 4)),
}
F32_ENTRIES = {"am_gemm_f32", "am_layernorm_f32", "am_head_post_f32", "am_attention_f32", "am_flow_step_f32"}


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


class TorchBackend:
    """HipF32Backend's four methods, and ops.flow_step for an fp32 velocity, as plain torch fp32 statements on CPU tensors, written
    from the contracts in include/actionmesh_amd.h (same in-place and aliasing behaviour)."""

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
        if out is None:
            return y
        out.copy_(y)
        return out

    def layernorm(self, x, w, b, eps, out=None):
        self._count("am_layernorm_f32")
        y = F.layer_norm(x, (x.shape[-1],), w, b, eps)
        if out is None:
            return y
        assert out.data_ptr() != x.data_ptr()
        out.copy_(y)
        return out

    def head_post(self, x, heads, w, off, head_stride, eps, rope=None, rows_per_frame=1):
        self._count("am_head_post_f32")
        rows = x.shape[0]
        for h in range(heads):
            c = x[:, off + h * head_stride: off + h * head_stride + HD]
            y = c * torch.rsqrt(c.pow(2).mean(-1, keepdim=True) + eps) * w
            if rope is not None:
                frame = torch.arange(rows) // rows_per_frame
                cs, sn = (t[frame].repeat_interleave(2, dim=1) for t in rope)
                yr, yi = y.reshape(rows, HD // 2, 2).unbind(-1)
                y = y * cs + torch.stack([-yi, yr], dim=-1).flatten(1) * sn
            c.copy_(y)
        return x

    def attention(self, q, k, v, heads, sq, sk, q_hs, k_hs, v_hs, q_off, k_off, v_off):
        self._count("am_attention_f32")
        nseq = q.shape[0] // sq

        def split(t, s, off, hs):
            return torch.stack([t[:, off + h * hs: off + h * hs + HD] for h in range(heads)], 0).reshape(heads, nseq, s, HD).transpose(0, 1)
        o = F.scaled_dot_product_attention(split(q, sq, q_off, q_hs), split(k, sk, k_off, k_hs), split(v, sk, v_off, v_hs))
        return o.transpose(1, 2).reshape(nseq * sq, heads * HD).contiguous()

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


def setup(name, golden_dir, dev, backend=None, **model_kw):
    """The fixture, the fp32 model on `dev` (with `backend` in place of the HIP kernels when given) and the inputs."""
    from actionmesh_amd import HipDenoiser
    from oracle import denoiser_oracle as O
    g = np.load(os.path.join(golden_dir, f"{name}.npz"))
    sd = O.synthetic_state_dict(O.OracleConfig(**CASES[name]), seed=0)
    assert abs(O.state_dict_checksum(sd) - float(g["weights_checksum"])) <= 1e-12 * abs(float(g["weights_checksum"]))
    model = HipDenoiser(num_tokens_nominal=48, temporal_context_size=4, dtype="float32", **CASES[name], **model_kw)
    model.f32_backend = backend
    model.load_state_dict(sd)
    model.to(dev).eval()
    t = {k: torch.from_numpy(g[k]) for k in ("init_latent", "context", "mask", "framestep")}
    return g, model, t


def guidance():
    from actionmesh_amd import ClassifierFreeGuidance
    return ClassifierFreeGuidance(True, [[0, 1], [1, 1]], [7.5])


def check_forward(name, golden_dir, dev, backend=None):
    """One forward against `fwd_velocity_fp32`; the velocity is float32; the returned cache gives identical bits; another context tensor
    with equal values re-binds."""
    g, model, t = setup(name, golden_dir, dev, backend)
    x_in, c_in, m_in, f_in = guidance().cfg_at_inference(t["init_latent"], t["context"], t["mask"], t["framestep"])
    tt = torch.tensor([float(g["fwd_t"])]).expand(2)
    c_dev = c_in.to(dev)
    assert model.compute_kind() == "f32"
    v, cache = model.forward(x_in.to(dev), c_dev, f_in.to(dev), tt.to(dev), m_in.to(dev), None)
    assert v.shape == x_in.shape and v.dtype == torch.float32
    r = rel(v.cpu(), torch.from_numpy(g["fwd_velocity_fp32"]))
    print(f"{name}: fp32 forward rel-L2 vs the reference's fp32 velocity {r:.3e}")
    assert r <= BOUND, r
    v2, cache2 = model.forward(x_in.to(dev), c_dev, f_in.to(dev), tt.to(dev), m_in.to(dev), cache)
    assert cache2 is cache and torch.equal(v2, v)
    v3, cache3 = model.forward(x_in.to(dev), c_in.to(dev).clone(), f_in.to(dev), tt.to(dev), m_in.to(dev), cache)
    assert cache3 is not cache and torch.equal(v3, v)
    return model, r


def check_loop(name, golden_dir, dev, backend=None, split=False):
    """The sampler loop: every step against `loop_latents_fp32` (split_cfg_batch: the final latents against `loop_final_split_cfg_fp32`),
    the conditioning frame bit-untouched."""
    from actionmesh_amd import HipSchedulerFlow
    g, model, t = setup(name, golden_dir, dev, backend)
    steps = int(g["steps"])
    # cuda_autocast_dt=True must change nothing for an fp32 model: the reference in fp32 has no autocast region to round dt in
    sched = HipSchedulerFlow(num_inference_steps=steps, shift=3.0, is_additive=True, split_cfg_batch=split, cuda_autocast_dt=True)
    ref = torch.from_numpy(g["loop_latents_fp32"])
    got = []
    for lat, _t in sched._flow_sample(model, guidance(), t["init_latent"].clone().to(dev), t["context"].to(dev), device=dev,
                                      mask=t["mask"].to(dev), framestep=t["framestep"].to(dev)):
        got.append(lat.clone().cpu())
    assert len(got) == steps
    curve = []
    for i in range(steps):
        assert got[i].dtype == torch.float32
        assert torch.equal(got[i][0, 0], t["init_latent"][0, 0]), "conditioning frame must stay untouched"
        curve.append(rel(got[i], ref[i]))
    final = rel(got[-1], torch.from_numpy(g["loop_final_split_cfg_fp32"])) if split else curve[-1]
    print(f"{name} (split_cfg_batch={split}): per-step latents rel-L2 vs the reference's fp32 loop " + " ".join(f"{c:.2e}" for c in curve)
          + (f"; final vs its split run {final:.3e}" if split else ""))
    if not split:
        assert max(curve) <= BOUND, curve
    assert final <= BOUND, final
    return model, curve, final
