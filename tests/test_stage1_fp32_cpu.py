"""HipDenoiser(dtype="float32") without a GPU: the orchestration of actionmesh_amd/denoiser_f32.py runs on torch-CPU restatements of its five
kernels (tests/_f32_backend.TorchBackend) against the fp32 values of the reference's own modules, and the declarations, refusals and
switches that reach the mode are checked.  The same assertions run on the kernels in tests/test_stage1_fp32_gpu.py.

Bound: rel-L2 <= 2e-5 (tests/_stage1_fp32.py).  Measured with the restatements (torch 2.x CPU kernels): 0.0 everywhere - tiny_inflated and
tiny_mixed, the forward, every step of the loop, the split_cfg_batch final latents: the stacked projections and the split linear_skip
give torch's own bits here, as the oracle's fp32 forward does."""
import os
import re

import pytest
import torch

import _stage1_fp32 as S
from test_dropin_cpu import reference_pipeline  # noqa: F401  (fixture: the reference's own pipeline module with stubbed heavy deps)

CPU = torch.device("cpu")


@pytest.fixture
def torch_flow_step(monkeypatch):
    """The sampler's CFG + Euler launch (ops.flow_step -> am_flow_step_f32 for an fp32 velocity) on the restatement."""
    import actionmesh_amd.scheduler as sched
    backend = S.TorchBackend()
    monkeypatch.setattr(sched.ops, "flow_step", backend.flow_step)
    return backend


@pytest.mark.parametrize("name", list(S.CASES))
def test_forward_against_the_reference_fp32_velocity(golden_dir, name):
    backend = S.TorchBackend()
    model, _ = S.check_forward(name, golden_dir, CPU, backend)
    assert model._engine.kind == "f32" and model._engine.entry_counts() == backend.calls
    assert set(backend.calls) == S.F32_ENTRIES - {"am_flow_step_f32"}


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("name", list(S.CASES))
def test_sampler_loop_against_the_reference_fp32_latents(golden_dir, torch_flow_step, name, split):
    S.check_loop(name, golden_dir, CPU, S.TorchBackend(), split=split)
    assert torch_flow_step.calls["am_flow_step_f32"] > 0


def test_entry_points_are_declared_and_bound():
    from actionmesh_amd import _lib as L
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "actionmesh_amd.h")).read()
    for name in ("am_head_post_f32", "am_flow_step_f32"):
        assert name in L.SYMBOLS and re.search(rf"\b{name}\(", hdr), name
    assert L.ABI_VERSION == 2
    assert L.is_f32(torch.float32) and L.is_f32("float32") and not L.is_f32(torch.bfloat16) and not L.is_f32("float16")


def test_options_that_cannot_apply_are_refused(monkeypatch):
    from actionmesh_amd import HipDenoiser
    kw = dict(S.CASES["tiny_mixed"], dtype=torch.float32)
    with pytest.raises(ValueError, match="process_group"):
        HipDenoiser(process_group=object(), **kw)
    with pytest.raises(ValueError, match="use_graph"):
        HipDenoiser(use_graph=True, **kw)
    for attn in ("fp8", "fp8_fast"):
        with pytest.raises(ValueError, match="attn_dtype"):
            HipDenoiser(attn_dtype=attn, **kw)
    monkeypatch.setenv("ACTIONMESH_AMD_GRAPH", "1")             # the environment switch is ignored in this mode, not refused
    m = HipDenoiser(**kw)
    assert m.fp32 and not m.use_graph and m.compute_kind() == "f32"
    assert HipDenoiser(**S.CASES["tiny_mixed"]).use_graph        # ... and still read by a 16-bit model


def test_a_16_bit_model_still_reports_its_kind(monkeypatch):
    """compute_kind(): 'bf16' / 'f16' for a 16-bit model as before - pinned, or from the caller's autocast region (the reference pipeline
    runs Stage I inside one, pipeline.py:671) - and 'f32' for the fp32 model whatever that region says."""
    from actionmesh_amd import HipDenoiser
    kw = S.CASES["tiny_mixed"]
    assert HipDenoiser(**kw).compute_kind() == "bf16" and not HipDenoiser(**kw).fp32
    assert HipDenoiser(dtype="bfloat16", **kw).compute_kind() == "bf16"
    assert HipDenoiser(dtype=torch.float16, **kw).compute_kind() == "f16"
    for spelling in ("float32", "fp32", "f32", torch.float32):
        assert HipDenoiser(dtype=spelling, **kw).compute_kind() == "f32"
    with pytest.raises(ValueError):
        HipDenoiser(dtype="float64", **kw)
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)          # inside torch.autocast("cuda", dtype=torch.float16)
    monkeypatch.setattr(torch, "get_autocast_dtype", lambda *a: torch.float16)
    assert HipDenoiser(**kw).compute_kind() == "f16"
    assert HipDenoiser(dtype="float32", **kw).compute_kind() == "f32"


def test_cli_stage1_fp32_flag():
    from actionmesh_amd import cli
    ours, rest = cli.split_args(["--stage1-fp32", "--", "--fast"])
    assert ours.stage1_fp32 and rest == ["--fast"]
    assert not cli.split_args(["--", "--fast"])[0].stage1_fp32            # off by default
    for bad in (["--stage1-fp32", "--attn-dtype", "fp8"], ["--stage1-fp32", "--backend", "reference"]):
        with pytest.raises(SystemExit) as e:
            cli.split_args(bad)
        assert e.value.code == 2                                          # argparse's usage error


@pytest.mark.skipif(not os.path.isdir("/root/reference/actionmesh"), reason="reference not present")
def test_install_stage1_fp32_binds_and_unbinds(reference_pipeline):  # noqa: F811
    P = reference_pipeline
    from actionmesh_amd import HipDenoiser, dropin
    original = P.ActionMeshDenoiser
    kw = S.CASES["tiny_mixed"]
    dropin.install()
    try:
        assert not P.ActionMeshDenoiser(**kw).fp32                        # off by default
        dropin.install_stage1_fp32()
        dropin.install_stage1_fp32()                                      # idempotent
        cls = P.ActionMeshDenoiser
        assert issubclass(cls, HipDenoiser) and cls.__name__ == "HipDenoiser"
        assert cls(**kw).fp32 and cls(**kw).compute_kind() == "f32"
        assert not cls(dtype="bfloat16", **kw).fp32
    finally:
        dropin.uninstall()
    assert P.ActionMeshDenoiser is original
    dropin.install_stage1_fp32()                                          # on its own: install() with its defaults first
    try:
        assert P.ActionMeshDenoiser(**kw).fp32
        dropin.install()                                                  # a later install() takes it back
        assert not P.ActionMeshDenoiser(**kw).fp32
    finally:
        dropin.uninstall()
    assert P.ActionMeshDenoiser is original
    dropin.install(attn_dtype="fp8")
    try:
        with pytest.raises(ValueError, match="attn_dtype"):
            dropin.install_stage1_fp32()
    finally:
        dropin.uninstall()
