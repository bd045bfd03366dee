"""HipAutoencoder(exact_fp32=True) without a GPU: the orchestration of actionmesh_amd/autoencoder_f32.py runs on torch-CPU restatements of
its six kernels (tests/_f32_backend.TorchBackend) against the reference's own fp32 displacement and the oracle, and the declarations,
refusals and switches that reach the mode are checked.  The same assertions run on the kernels in tests/test_stage2_fp32_gpu.py.

Bound: rel-L2 <= 2e-5 (tests/_stage2_fp32.py).  Measured with the restatements (torch CPU kernels): ae_tiny 5.0e-7, ae_arch 7.0e-7; the cases
against the oracle 4.1e-7 .. 4.7e-7, the window loop's vertices 4.1e-7 .. 4.8e-7 - not 0.0 as in Stage I: F.scaled_dot_product_attention sums the frame-major key order in another
order than the reference's [latents | alphas] one."""
import json
import os
import re

import pytest
import torch

import _stage2_fp32 as S
from test_dropin_cpu import REF, reference_pipeline  # noqa: F401  (fixture: the reference's own pipeline module with stubbed heavy deps)

CPU = torch.device("cpu")
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "actionmesh")), reason="reference not present")


@pytest.mark.parametrize("name", ["ae_tiny", "ae_arch"])
def test_forward_against_the_reference_fp32_displacement(golden_dir, name):
    backend = S.TorchBackend()
    model, cfg, sd, t, d, r = S.check_fixture(name, golden_dir, CPU, backend)
    B, T_out = t["target_alphas"].shape
    assert model.entry_counts() == backend.calls == S.expected_counts(cfg.num_layers, T_out, B)
    assert set(backend.calls) == S.F32_ENTRIES


@pytest.mark.parametrize("case", S.CASES, ids=[c[0] for c in S.CASES])
def test_cases_the_fixtures_do_not_reach(case):
    S.check_case(case, CPU, S.TorchBackend())


def test_no_state_leaks_between_targets():
    S.check_no_state_between_targets(CPU, S.TorchBackend)


def test_vertex_animation_passes_the_exact_mode_through():
    S.check_vertex_animation(CPU, S.TorchBackend())


def test_entry_point_is_declared_and_bound():
    from actionmesh_amd import _lib as L
    from actionmesh_amd import ops
    from actionmesh_amd.f32_backend import HipF32Backend
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "actionmesh_amd.h")).read()
    assert "am_rope_f32" in L.SYMBOLS and re.search(r"\bam_rope_f32\(", hdr)
    assert L.ABI_VERSION == 2 and callable(ops.rope_f32)
    for method in ("rope", "point_embed", "displacement"):
        assert callable(getattr(HipF32Backend, method))


def test_the_switch_and_what_it_implies(monkeypatch):
    from actionmesh_amd import HipAutoencoder
    kw = dict(width=256, num_layers=1, num_attention_heads=2)
    m = HipAutoencoder(exact_fp32=True, **kw)
    assert m.exact_fp32 and m.cross_fp32 and m.residual_fp32 and m.compute_kind() == "f32"
    assert HipAutoencoder(exact_fp32=True, residual_fp32=True, cross_fp32=True, **kw).exact_fp32
    for bad in (dict(residual_fp32=False), dict(cross_fp32=False), dict(residual_fp32=False, cross_fp32=False)):
        with pytest.raises(ValueError, match="exact_fp32"):
            HipAutoencoder(exact_fp32=True, **bad, **kw)
    # the 16-bit modes keep their defaults and their kinds, and float32 as a dtype stays refused - now with a pointer to the switch
    d = HipAutoencoder(**kw)
    assert not d.exact_fp32 and d.residual_fp32 and not d.cross_fp32 and d.compute_kind() == "bf16"
    assert not HipAutoencoder(residual_fp32=False, **kw).residual_fp32 and HipAutoencoder(cross_fp32=True, **kw).cross_fp32
    with pytest.raises(ValueError, match="bfloat16 or float16.*exact_fp32=True"):
        HipAutoencoder(dtype=torch.float32, **kw)
    with pytest.raises(ValueError, match="bfloat16 or float16"):
        HipAutoencoder(dtype="float64", **kw)
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)          # inside torch.autocast("cuda", dtype=torch.float16)
    monkeypatch.setattr(torch, "get_autocast_dtype", lambda *a: torch.float16)
    assert HipAutoencoder(**kw).compute_kind() == "f16" and HipAutoencoder(exact_fp32=True, **kw).compute_kind() == "f32"


def test_from_pretrained_constructs_the_exact_mode_on_the_cpu(tmp_path, golden_dir):
    from safetensors.torch import save_file
    from actionmesh_amd import HipAutoencoder
    cfg, sd, t = S.fixture(golden_dir, "ae_tiny")
    (tmp_path / "config.json").write_text(json.dumps(dict(width=cfg.width, num_layers=cfg.num_layers,
                                                          num_attention_heads=cfg.num_attention_heads, verbose=False)))
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "model.safetensors"))
    m = HipAutoencoder.from_pretrained(str(tmp_path), exact_fp32=True)
    assert m.exact_fp32 and m.compute_kind() == "f32" and m.device == CPU and (m.width, m.num_layers) == (cfg.width, cfg.num_layers)
    with pytest.raises(RuntimeError):      # no CPU path of its own: only a backend of the caller's runs off the device
        S.run(m, t, CPU)
    m.f32_backend = S.TorchBackend()
    assert S.rel(S.run(m, t, CPU), t["displacement_fp32"]) <= S.BOUND


def test_cli_stage2_fp32_flag():
    from actionmesh_amd import cli
    ours, rest = cli.split_args(["--stage2-hip", "--stage2-fp32", "--", "--fast"])
    assert ours.stage2_fp32 and ours.stage2_hip and rest == ["--fast"]
    assert not cli.split_args(["--stage2-hip", "--", "--fast"])[0].stage2_fp32            # off by default
    with pytest.raises(SystemExit) as e:
        cli.split_args(["--stage2-fp32"])
    assert e.value.code == 2                                                              # argparse's usage error


@needs_reference
def test_install_stage2_fp32_binds_and_unbinds(reference_pipeline):  # noqa: F811
    P = reference_pipeline
    from actionmesh_amd import HipAutoencoder, dropin
    original = P.ActionMeshAutoencoder
    kw = dict(width=256, num_layers=1, num_attention_heads=2)
    with pytest.raises(RuntimeError, match="stage2=True"):
        dropin.install_stage2_fp32()                                      # nothing installed
    dropin.install()
    try:
        with pytest.raises(RuntimeError, match="stage2=True"):
            dropin.install_stage2_fp32()                                  # installed, but Stage II is the reference's
        assert P.ActionMeshAutoencoder is original
    finally:
        dropin.uninstall()
    dropin.install(stage2=True)
    try:
        assert not P.ActionMeshAutoencoder(**kw).exact_fp32               # off by default
        dropin.install_stage2_fp32()
        dropin.install_stage2_fp32()                                      # idempotent
        cls = P.ActionMeshAutoencoder
        assert issubclass(cls, HipAutoencoder) and cls.__name__ == "HipAutoencoder"
        m = cls(**kw)
        assert m.exact_fp32 and m.cross_fp32 and m.compute_kind() == "f32"
        assert not cls(exact_fp32=False, **kw).exact_fp32
        dropin.install(stage2=True)                                       # a later install() takes it back
        assert not P.ActionMeshAutoencoder(**kw).exact_fp32
    finally:
        dropin.uninstall()
    assert P.ActionMeshAutoencoder is original
