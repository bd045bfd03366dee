"""What tests/test_stage2_fp32_cpu.py and tests/test_stage2_fp32_gpu.py share: torch-CPU restatements of the kernels behind the interface
of `actionmesh_amd.f32_backend.HipF32Backend` as the exact-fp32 Stage II uses it (tests/_f32_backend.TorchBackend: Stage I's methods,
am_rope_f32, am_point_embed_f32 and am_displacement_f32, written from the contracts in include/actionmesh_amd.h), so that the orchestration of
HipAutoencoder(exact_fp32=True) runs without a device, and the assertions both files make - on the restatements in one, on the
kernels in the other.

The bound throughout is rel-L2 <= 2e-5: against `displacement_fp32` of tests/golden/ae_tiny.npz / ae_arch.npz (the reference's own
unmodified ActionMeshAutoencoder in fp32) and, for the cases the fixtures do not reach, against oracle.autoencoder_oracle computed in
the test.  It is the bound tests/_stage1_fp32.py holds the same kernels to through Stage I's 21 blocks; Stage II has 17 and ends in a
sigmoid of slope <= 1/2."""
import os

import numpy as np
import torch

import _stage1_fp32 as S1
from oracle import autoencoder_oracle as AO

BOUND = S1.BOUND
HD = S1.HD
TorchBackend = S1.TorchBackend
rel = S1.rel
F32_ENTRIES = {"am_gemm_f32", "am_layernorm_f32", "am_rope_f32", "am_attention_f32", "am_point_embed_f32", "am_displacement_f32"}
SMALL = dict(width=256, num_layers=2, num_attention_heads=2, latent_channels=64)          # 2 + 1 blocks


def fixture(golden_dir, name):
    """(AEConfig, state dict, tensors) of tests/golden/<name>.npz, the weights regenerated from the seed and pinned by the checksum."""
    g = np.load(os.path.join(golden_dir, f"{name}.npz"))
    width, layers, heads, latent = (int(v) for v in g["config"])
    cfg = AO.AEConfig(width=width, num_layers=layers, num_attention_heads=heads, latent_channels=latent)
    sd = AO.synthetic_state_dict(cfg, seed=0)
    assert abs(AO.state_dict_checksum(sd) - float(g["weights_checksum"])) <= 1e-12 * abs(float(g["weights_checksum"]))
    t = {k: torch.from_numpy(g[k]) for k in ("latent", "framestep", "source_alpha", "target_alphas", "query", "displacement_fp32")}
    return cfg, sd, t


def build(cfg, sd, dev, backend=None, **kw):
    """HipAutoencoder for `cfg` on `dev`; exact_fp32 unless `kw` says otherwise (`backend` in place of the HIP kernels when given)."""
    from actionmesh_amd import HipAutoencoder
    kw.setdefault("exact_fp32", True)
    m = HipAutoencoder(in_extra_channels=cfg.in_extra_channels, width=cfg.width, num_layers=cfg.num_layers,
                       num_attention_heads=cfg.num_attention_heads, latent_channels=cfg.latent_channels,
                       embed_include_pi=cfg.embed_include_pi, **kw)
    m.f32_backend = backend
    m.load_state_dict(sd)
    return m.to(dev).eval()


def run(model, t, dev, **kw):
    """One forward on the fixture-shaped tensors `t`, the displacement on the CPU."""
    d = model(t["latent"].to(dev), t["framestep"], t["source_alpha"], t["target_alphas"], t["query"].to(dev), **kw)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return d.cpu()


def check_fixture(name, golden_dir, dev, backend=None):
    """The exact forward against `displacement_fp32`: fp32 out, rel-L2 <= BOUND (max-abs printed, not bounded), the callback in order."""
    cfg, sd, t = fixture(golden_dir, name)
    model = build(cfg, sd, dev, backend)
    assert model.compute_kind() == "f32" and model.exact_fp32 and model.cross_fp32 and model.residual_fp32
    seen = []
    d = run(model, t, dev, step_callback=lambda i, n: seen.append((i, n)))
    ref = t["displacement_fp32"]
    T_out = ref.shape[1]
    assert d.shape == ref.shape and d.dtype == torch.float32 and seen == [(i + 1, T_out) for i in range(T_out)]
    r, mx = rel(d, ref), float((d - ref).abs().max())
    print(f"{name}: exact fp32 displacement rel-L2 {r:.3e}, max abs {mx:.3e} vs the reference's fp32 displacement")
    assert r <= BOUND, r
    assert float(d.abs().max()) <= 1.0
    return model, cfg, sd, t, d, r


def expected_counts(NL, T_out, B):
    """Launches per entry point of one exact forward (autoencoder_f32.forward_f32)."""
    return {"am_gemm_f32": 2 + T_out * (4 * NL + 6), "am_layernorm_f32": T_out * (2 * NL + 4), "am_rope_f32": T_out * NL,
            "am_attention_f32": T_out * (NL + 1), "am_point_embed_f32": 1, "am_displacement_f32": T_out * B}


# the cases the fixtures do not reach: (name, B, framesteps, N, V, T_out, in_extra_channels)
CASES = [
    ("two_entries_gapped_framesteps_v1", 2, [[0, 3, 4], [2, 5, 9]], 5, 1, 2, 3),          # T L = 18
    ("sequence_256_v255_one_target", 1, [[0, 1, 2, 3]], 63, 255, 1, 3),                   # T L = 256 exactly
    ("sequence_260_v257", 1, [[1, 2, 4, 7]], 64, 257, 2, 3),                              # T L = 260
    ("no_extra_channels", 2, [[0, 3, 4], [2, 5, 9]], 5, 7, 1, 0),                         # (B, V, 3) query
]


def case_inputs(B, framesteps, N, V, T_out, extra, seed=5):
    g = torch.Generator().manual_seed(seed + N + V)
    fs = torch.tensor(framesteps, dtype=torch.float32)
    T = fs.shape[1]
    q = torch.rand((B, V, 3), generator=g) * 2 - 1
    if extra:
        q = torch.cat([q, torch.nn.functional.normalize(torch.randn((B, V, extra), generator=g), dim=-1)], -1)
    return {"latent": torch.randn((B, T, N, 64), generator=g), "framestep": fs, "source_alpha": torch.rand((B,), generator=g),
            "target_alphas": torch.rand((B, T_out), generator=g), "query": q}


def check_case(case, dev, backend=None):
    name, B, framesteps, N, V, T_out, extra = case
    cfg = AO.AEConfig(in_extra_channels=extra, **SMALL)
    sd = AO.synthetic_state_dict(cfg, seed=2)
    t = case_inputs(B, framesteps, N, V, T_out, extra)
    ref = AO.autoencoder_forward(sd, cfg, t["latent"], t["framestep"], t["source_alpha"], t["target_alphas"], t["query"])
    model = build(cfg, sd, dev, backend)
    seen = []
    d = run(model, t, dev, step_callback=lambda i, n: seen.append((i, n)))
    assert d.shape == (B, T_out, V, 3) and d.dtype == torch.float32 and seen == [(i + 1, T_out) for i in range(T_out)]
    r = rel(d, ref)
    print(f"{name}: exact fp32 displacement rel-L2 {r:.3e}, max abs {float((d - ref).abs().max()):.3e} vs the oracle")
    assert r <= BOUND, (name, r)
    assert model.entry_counts() == expected_counts(cfg.num_layers, T_out, B), model.entry_counts()
    return r


def check_no_state_between_targets(dev, backend_factory=lambda: None):
    """Target i of a T_out = 3 call is, bit for bit, the T_out = 1 call with that alpha (a base stream or a query stream modified in place
    would show here), and two identical calls give the same bits."""
    cfg = AO.AEConfig(**SMALL)
    sd = AO.synthetic_state_dict(cfg, seed=2)
    t = case_inputs(1, [[0, 2, 3]], 6, 33, 3, 3)
    model = build(cfg, sd, dev, backend_factory())
    d = run(model, t, dev)
    assert torch.equal(run(model, t, dev).view(torch.int32), d.view(torch.int32)), "two identical calls differ"
    for i in range(3):
        one = dict(t, target_alphas=t["target_alphas"][:, i:i + 1].contiguous())
        di = run(model, one, dev)
        assert torch.equal(di[:, 0].view(torch.int32), d[:, i].view(torch.int32)), f"target {i} depends on the targets around it"
    assert not torch.equal(d[:, 0], d[:, 1])


def check_vertex_animation(dev, backend=None):
    """generate_vertex_animation with an exact_fp32 autoencoder, one window of ae_tiny's size: vertex features fp32 in, vertices fp32
    out, within the bound of the oracle's."""
    from actionmesh_amd import windows as W
    from oracle import windows_oracle as WO
    cfg = AO.AEConfig(**SMALL)
    sd = AO.synthetic_state_dict(cfg, seed=1)
    g = torch.Generator().manual_seed(9)
    T, N, D, V = 4, 16, 64, 50
    ts = torch.arange(T, dtype=torch.float32)
    lat = torch.randn((T, N, D), generator=g)
    verts = torch.rand((V, 3), generator=g) * 1.6 - 0.8
    feats = lambda v: torch.cat([v, torch.nn.functional.normalize(v + 0.05, dim=-1)], dim=-1)
    model = build(cfg, sd, dev, backend, temporal_context_size=T)
    bank = W.LatentBank(empty_dims=(N, D), device=str(dev)); bank.update(ts, lat)
    vbank = W.LatentBank(empty_dims=(V, 3), device=str(dev)); vbank.update(ts[:1], verts[None])
    W.generate_vertex_animation(model, bank, vbank, feats, 0, T, T - 1, device=dev)
    got, got_ts = vbank.get_ordered()
    ref_bank = WO.ListLatentBank((N, D)); ref_bank.update(ts, lat)

    def decode(latents, wts, sa, ta, src):
        return torch.clamp(AO.autoencoder_forward(sd, cfg, latents, wts, sa, ta, feats(src)[None]), -1.0, 1.0)[0]
    meshes = WO.generate_mesh_animation(decode, ref_bank, {0.0: verts}, 0, T, T - 1)
    assert got.dtype == torch.float32 and got_ts.tolist() == sorted(meshes) == ts.tolist()
    assert torch.equal(got[0].cpu(), verts)
    errs = [rel(got[i].cpu(), meshes[float(i)]) for i in range(1, T)]
    print("vertex animation: vertices rel-L2 vs the oracle's " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= BOUND, errs
