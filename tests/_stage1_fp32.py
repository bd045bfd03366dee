"""What tests/test_stage1_fp32_cpu.py and tests/test_stage1_fp32_gpu.py share: the tiny fixtures' cases, torch-CPU restatements of the five
kernels - the four of the forward behind the interface of `actionmesh_amd.f32_backend.HipF32Backend`, and the sampler's CFG + Euler
step (tests/_f32_backend.TorchBackend) - so that the orchestration of HipDenoiser(dtype="float32") runs without a device, and the assertions both files make on `tiny_inflated` / `tiny_mixed` - on the restatements in one, on the kernels in
the other.

The bound throughout is rel-L2 <= 2e-5 against the fp32 values of the reference's own modules (tests/golden/tiny_*.npz): the statement
tests/test_fp32_path_gpu.py makes for the 24-layer fp32 encoder against an independent fp32 implementation."""
import os

import numpy as np
import torch

from _f32_backend import HD, TorchBackend  # noqa: F401  (the one restatement; both test files reach it through this module)

BOUND = 2e-5
CASES = {
    "tiny_inflated": dict(in_channels=64, num_layers=5, num_attention_heads=2, width=256,
                          mlp_ratio=4.0, cross_attention_dim=64, inflated_layers=(0, 1, 2, 3, 4)),
    "tiny_mixed": dict(in_channels=64, num_layers=5, num_attention_heads=2, width=256,
                       mlp_ratio=4.0, cross_attention_dim=64, inflated_layers=(0, 1, 3, 4)),
}
F32_ENTRIES = {"am_gemm_f32", "am_layernorm_f32", "am_head_post_f32", "am_attention_f32", "am_flow_step_f32"}


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


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
