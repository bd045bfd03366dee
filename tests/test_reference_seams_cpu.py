"""Seams S1 / S2 against the REFERENCE's own classes (CPU).  2. and the overlay check need the reference checkout (REF) and are
skipped where it is absent; 1. runs everywhere.

1. `inspect.signature` equality of the drop-in surfaces with the reference classes they replace, as recorded from the reference in
   tests/golden/reference_signatures.json (oracle/make_golden_signatures.py; re-checked against the live classes where present).
2. The reference's OWN `SchedulerFlow` + `ClassifierFreeGuidance` objects (not a restated loop) drive `HipDenoiser`
   through the S2 protocol - keyword call, opaque `freqs_rot` cache handed back, batched and `split_cfg_batch=True`
   (one forward per CFG branch re-using branch 0's cache object, scheduler.py:159-168).  There is no GPU here, so the
   engine behind HipDenoiser is an oracle-backed stand-in with HipEngine's interface; what is under test is the HOST
   logic of HipDenoiser (window binding tied to the context, masked time, CFG order), which is identical on the GPU.
   The result must equal the fixture the reference's own model produced.
"""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
HAVE_REF = os.path.isdir(os.path.join(REF, "actionmesh"))
needs_ref = pytest.mark.skipif(not HAVE_REF, reason="reference not present")


def _ref():
    for p in (os.path.join(ROOT, "oracle", "diffusers_shim"), REF):
        if p not in sys.path:
            sys.path.insert(0, p)
    from actionmesh.model.temporal_denoiser import ActionMeshDenoiser
    from actionmesh.scheduler.guidance import ClassifierFreeGuidance
    from actionmesh.scheduler.scheduler import SchedulerFlow
    return ActionMeshDenoiser, ClassifierFreeGuidance, SchedulerFlow


def _sig(fn):
    s = inspect.signature(fn)
    return [(n, p.kind, p.default) for n, p in s.parameters.items()]


def _recorded_signatures(golden_dir):
    import json
    with open(os.path.join(golden_dir, "reference_signatures.json")) as f:
        return json.load(f)


def _rec(fn):
    """(name, kind, repr(default) or None) - the form tests/golden/reference_signatures.json records."""
    from oracle.make_golden_signatures import signature_record
    return [tuple(p) for p in signature_record(fn)]


def test_signatures_equal_the_references(golden_dir):
    import actionmesh_amd as A
    rec = {cls: {m: [tuple(p) for p in sig] for m, sig in methods.items()} for cls, methods in _recorded_signatures(golden_dir).items()}
    RefSched, RefCFG, RefDenoiser = rec["SchedulerFlow"], rec["ClassifierFreeGuidance"], rec["ActionMeshDenoiser"]
    for name in ("denoise", "get_noise", "get_schedule", "_flow_sample", "_compute_timesteps"):
        assert _rec(getattr(A.HipSchedulerFlow, name)) == RefSched[name], name
    for name in ("get_unobserved_mask", "cfg_at_inference", "aggregate_cfg"):
        assert _rec(getattr(A.ClassifierFreeGuidance, name)) == RefCFG[name], name
    assert _rec(A.HipDenoiser.forward) == RefDenoiser["forward"]
    # constructors: every reference field, same order and defaults (ours may append optional fields)
    ours, ref = _rec(A.HipSchedulerFlow.__init__), RefSched["__init__"]
    assert ours[:len(ref)] == ref and all(d is not None for _, _, d in ours[len(ref):])
    ours, ref = _rec(A.ClassifierFreeGuidance.__init__), RefCFG["__init__"]
    assert [n for n, _, _ in ours] == [n for n, _, _ in ref]
    ours, ref = _rec(A.HipDenoiser.__init__), RefDenoiser["__init__"]
    assert all(d is not None for _, _, d in ours[len(ref):])
    for (n, k, d), (rn, rk, rd) in zip(ours, ref):
        assert (n, k) == (rn, rk)
        if "factory" not in str(rd):        # dataclass default_factory (inflated_layers): ours resolves None the same way
            assert d == rd, n


@needs_ref
def test_recorded_signatures_are_the_references(golden_dir):
    """The fixture above is what the reference's classes say now (regenerate with oracle/make_golden_signatures.py)."""
    import importlib
    from oracle.make_golden_signatures import SURFACES
    _ref()
    for cls, methods in _recorded_signatures(golden_dir).items():
        mod, name, _ = SURFACES[cls]
        klass = getattr(importlib.import_module(mod), name)
        for m, sig in methods.items():
            assert _rec(getattr(klass, m)) == [tuple(p) for p in sig], (cls, m)


class StandInEngine:
    """HipEngine's interface over the fp32 CPU oracle (tests only)."""

    def __init__(self, hp, sd):
        from oracle import denoiser_oracle as O
        self.O, self.sd = O, sd
        self.cfg = O.OracleConfig(in_channels=hp["in_channels"], num_layers=hp["num_layers"],
                                  num_attention_heads=hp["num_attention_heads"], width=hp["width"],
                                  mlp_ratio=hp["mlp_ratio"], cross_attention_dim=hp["cross_attention_dim"],
                                  inflated_layers=tuple(hp["inflated_layers"]))
        self.device, self.world, self.rank, self.kind = torch.device("cpu"), 1, 0, "bf16"
        self.binds = 0

    def fits(self, *a):
        return True

    def close(self):
        pass

    def set_context(self, ctx_local, cos, sin, ctx_zero=None, shared_prefix=False):
        # the stand-in ignores the exact-shortcut hints (HipEngine forwards them to am_set_branch_hints); what reaches it must
        # describe the context it is given
        assert ctx_zero is None or [bool(z) for z in ctx_zero] == [not bool(c.any()) for c in ctx_local]
        assert not shared_prefix
        self.ctx = ctx_local.clone()
        self.cos, self.sin = cos.repeat_interleave(2, dim=1), sin.repeat_interleave(2, dim=1)
        self.binds += 1

    def forward(self, x, t_bt):
        from test_sharding_gloo import OracleEngine
        from actionmesh_amd.sharding import FrameShardPlan
        B, T, N, _ = x.shape
        assert self.ctx.shape[:2] == (B, T), "forward against a window bound for another batch"
        e = OracleEngine(self.sd, self.cfg, FrameShardPlan(T, 1, 0), self.ctx, self.cos, self.sin, B, N)
        e.begin(x, t_bt)
        for i in range(self.cfg.num_layers):
            e.layer_pre(i)
            e.layer_post(i)
        return e.end()


@needs_ref
@pytest.mark.parametrize("split", [False, True])
def test_reference_scheduler_object_drives_hipdenoiser(golden_dir, split, monkeypatch):
    import actionmesh_amd as A
    from oracle import denoiser_oracle as O
    _, RefCFG, RefSched = _ref()
    kw = dict(in_channels=64, num_layers=5, num_attention_heads=2, width=256, mlp_ratio=4.0, cross_attention_dim=64,
              inflated_layers=(0, 1, 2, 3, 4))
    g = np.load(os.path.join(golden_dir, "tiny_inflated.npz"))
    sd = O.synthetic_state_dict(O.OracleConfig(**kw), seed=0)
    model = A.HipDenoiser(num_tokens_nominal=48, temporal_context_size=4, **kw)
    model.load_state_dict(sd)
    engine = StandInEngine(model.hyper_params(), sd)
    monkeypatch.setattr(model, "_ensure_engine", lambda *a, **k: (setattr(model, "_engine", engine), engine)[1])
    steps = int(g["steps"])
    sched = RefSched(num_inference_steps=steps, num_train_timesteps=1000, shift=3.0, is_additive=True, split_cfg_batch=split)
    cfgd = RefCFG(inference_enabled=True, guidance_at_inference=[[0, 1], [1, 1]], guidance_scales=[7.5])
    t = {k: torch.from_numpy(g[k]) for k in ("init_latent", "context", "mask", "framestep")}
    out = sched.denoise(model, cfgd, init_latent=t["init_latent"].clone(), context=t["context"], device="cpu",
                        disable_prog=True, mask=t["mask"], framestep=t["framestep"])
    ref = torch.from_numpy(g["loop_final_split_cfg_fp32"] if split else g["loop_latents_fp32"][-1])
    err = float((out - ref).abs().max())
    assert torch.allclose(out, ref, rtol=1e-4, atol=1e-4), err
    # split: every call carries another context slice, so the window is re-bound per call (reusing branch
    # 0's zeroed-context K/V for the conditioned branch silently dropped the image conditioning); batched: cfg_at_inference
    # builds a new context tensor every step, and a window is never reused across different tensors
    assert engine.binds == (2 * steps if split else steps)


def test_window_cache_is_reused_only_for_the_same_context(monkeypatch):
    import actionmesh_amd as A
    from oracle import denoiser_oracle as O
    kw = dict(in_channels=64, num_layers=1, num_attention_heads=2, width=256, mlp_ratio=4.0, cross_attention_dim=64,
              inflated_layers=(0,))
    sd = O.synthetic_state_dict(O.OracleConfig(**kw), seed=0)
    model = A.HipDenoiser(num_tokens_nominal=8, temporal_context_size=2, **kw)
    model.load_state_dict(sd)
    engine = StandInEngine(model.hyper_params(), sd)
    monkeypatch.setattr(model, "_ensure_engine", lambda *a, **k: (setattr(model, "_engine", engine), engine)[1])
    x, ctx = torch.randn(2, 2, 8, 64), torch.randn(2, 2, 5, 64)
    fs, t = torch.tensor([[0.0, 1.0]] * 2), torch.tensor([500.0, 500.0])
    v0, cache = model.forward(x, ctx, fs, t, None, None)
    v1, cache1 = model.forward(x, ctx, fs, t, None, cache)
    assert cache1 is cache and engine.binds == 1 and torch.equal(v0, v1)
    ctx.mul_(2.0)                                   # in-place edit of the same storage: torch bumps the version counter
    _, cache2 = model.forward(x, ctx, fs, t, None, cache)
    assert cache2 is not cache and engine.binds == 2
    _, cache3 = model.forward(x, ctx.clone(), fs, t, None, cache2)
    assert cache3 is not cache2 and engine.binds == 3
    _, cache4 = model.forward(x[:1], ctx[1:2], fs[:1], t[:1], None, cache3)      # a per-branch call (split_cfg_batch)
    assert cache4 is not cache3 and engine.binds == 4


@needs_ref
def test_overlays_cover_the_reference_presets():
    """One *_mi355x.yaml overlay per preset the reference CLI can pick (inference/video_to_animated_mesh.py:199-210); each derives
    from its preset, overrides ONLY keys the reference base config has, names importable classes whose dataclass fields cover what
    the reference YAML passes to the sampler / the guidance, and changes nothing else."""
    import importlib
    import yaml
    ref_dir = os.path.join(REF, "actionmesh", "configs")
    ov_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "actionmesh_amd", "configs")
    presets = sorted(f[:-5] for f in os.listdir(ref_dir) if f.endswith(".yaml"))
    assert presets == ["actionmesh", "actionmesh_fast", "actionmesh_fast_lowram", "actionmesh_lowram"]
    base = yaml.safe_load(open(os.path.join(ref_dir, "actionmesh.yaml")))
    cli = open(os.path.join(REF, "inference", "video_to_animated_mesh.py")).read()

    def leaves(d, prefix=()):
        for k, v in d.items():
            if isinstance(v, dict):
                yield from leaves(v, prefix + (k,))
            else:
                yield prefix + (k,), v

    for preset in presets:
        assert f'"{preset}.yaml"' in cli, f"the CLI no longer selects {preset}.yaml"
        ov = yaml.safe_load(open(os.path.join(ov_dir, f"{preset}_mi355x.yaml")))
        assert ov["defaults"] == [preset]
        over = {k: v for k, v in leaves({k: v for k, v in ov.items() if k != "defaults"})}
        assert set(over) == {("model", "scheduler", "_target_"), ("model", "cf_guidance", "_target_")}
        for path, target in over.items():
            node = base
            for k in path:
                assert k in node, f"{preset}_mi355x.yaml overrides {'.'.join(path)}, which actionmesh.yaml does not have"
                node = node[k]
            mod, cls = target.rsplit(".", 1)
            klass = getattr(importlib.import_module(mod), cls)
            ref_kwargs = {k for k in base[path[0]][path[1]] if not k.startswith("_")}
            preset_cfg = yaml.safe_load(open(os.path.join(ref_dir, f"{preset}.yaml")))
            ref_kwargs |= {k for k in (preset_cfg.get("model", {}) or {}).get(path[1], {}) if not k.startswith("_")}
            fields = set(inspect.signature(klass).parameters)
            assert ref_kwargs <= fields, f"{cls} lacks {ref_kwargs - fields} that {preset}.yaml passes"
