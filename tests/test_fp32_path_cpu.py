"""The exact-fp32 path without a GPU: the built libraries carry fp32-MFMA kernels (and nothing narrower in them, no scratch), the CLI
and drop-in options reach HipAutoencoder(cross_fp32=True), and the option combinations that cannot work are refused."""
import glob
import os
import re
import shutil
import subprocess

import pytest

from test_dropin_cpu import reference_pipeline  # noqa: F401  (fixture: the reference's own pipeline module with stubbed heavy deps)

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
FP32_KERNELS = ("gemm_f32_kernel", "attention_f32_kernel")


def _disassemble(path, tmp_path):
    shutil.copy(path, tmp_path / "lib.so")
    subprocess.run([OBJDUMP, "--offloading", "lib.so"], cwd=tmp_path, check=True, capture_output=True)
    objs = sorted(glob.glob(str(tmp_path / "lib.so.*gfx950")))
    assert objs, "no gfx950 code objects in the library"
    body, kernel = {}, None
    for o in objs:
        for line in subprocess.run([OBJDUMP, "-d", o], check=True, capture_output=True, text=True).stdout.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                kernel = m.group(1)
                body.setdefault(kernel, [])
            elif kernel is not None:
                body[kernel].append(line)
    return body


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_fp32_kernels_use_fp32_mfma_only(tmp_path, kind):
    """Every fp32 GEMM / attention kernel in the built library issues v_mfma_f32_32x32x2_f32 or v_mfma_f32_16x16x4_f32, no 16-bit or
    fp8 MFMA, and never touches scratch (no spills)."""
    from actionmesh_amd import _lib as L
    path = L.LIB_PATH if kind == "bf16" else L.LIB_PATH_F16
    if not (os.path.exists(path) and os.path.exists(OBJDUMP)):
        pytest.skip("library or llvm-objdump missing")
    body = _disassemble(path, tmp_path)
    found = {k: [n for n in body if k in n] for k in FP32_KERNELS}
    assert all(found.values()), found
    fp32_mfma = re.compile(r"v_mfma_f32_(32x32x2|16x16x4)_f32\b")
    for names in found.values():
        for n in names:
            mfma = [ln for ln in body[n] if "v_mfma" in ln]
            print(f"{kind} {n}: {len(mfma)} MFMA instructions")
            assert mfma and all(fp32_mfma.search(ln) for ln in mfma), (n, [ln for ln in mfma if not fp32_mfma.search(ln)][:3])
            assert not any("scratch_" in ln for ln in body[n]), f"{n} spills to scratch"


def test_entry_points_are_declared_and_bound():
    from actionmesh_amd import _lib as L
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "actionmesh_amd.h")).read()
    for name in ("am_gemm_f32", "am_attention_f32", "am_layernorm_f32", "am_point_embed_f32", "am_patchify_f32", "am_displacement_f32"):
        assert name in L.SYMBOLS and re.search(rf"\b{name}\(", hdr), name
    assert L.ABI_VERSION == 2


def test_cli_stage2_cross_fp32_flag():
    from actionmesh_amd import cli
    ours, rest = cli.split_args(["--stage2-hip", "--stage2-cross-fp32", "--", "--fast"])
    assert ours.stage2_hip and ours.stage2_cross_fp32 and rest == ["--fast"]
    ours, _ = cli.split_args(["--stage2-hip"])
    assert not ours.stage2_cross_fp32
    with pytest.raises(SystemExit) as e:
        cli.split_args(["--stage2-cross-fp32"])
    assert e.value.code == 2                               # argparse's usage error


@pytest.mark.skipif(not os.path.isdir("/root/reference/actionmesh"), reason="reference not present")
def test_install_binds_stage2_cross_fp32(reference_pipeline):  # noqa: F811
    P = reference_pipeline
    from actionmesh_amd import HipAutoencoder, dropin
    dropin.install(stage2=True, stage2_cross_fp32=True)
    try:
        cls = P.ActionMeshAutoencoder
        assert issubclass(cls, HipAutoencoder) and cls.__name__ == "HipAutoencoder"
        m = cls(width=256, num_layers=1, num_attention_heads=2)
        assert m.cross_fp32 and m.residual_fp32
        assert not cls(width=256, num_layers=1, num_attention_heads=2, cross_fp32=False).cross_fp32
    finally:
        dropin.uninstall()
    dropin.install(stage2=True)
    try:
        assert P.ActionMeshAutoencoder is HipAutoencoder
    finally:
        dropin.uninstall()
    with pytest.raises(ValueError, match="stage2"):
        dropin.install(stage2_cross_fp32=True)


def test_cross_fp32_needs_the_fp32_residual_stream():
    from actionmesh_amd._lib import HipLibraryMissing
    from actionmesh_amd.autoencoder import HipAutoencoder
    try:
        with pytest.raises(ValueError, match="residual_fp32"):
            HipAutoencoder(width=256, num_layers=1, num_attention_heads=2, cross_fp32=True, residual_fp32=False)
        assert not HipAutoencoder(width=256, num_layers=1, num_attention_heads=2).cross_fp32       # the default is unchanged
    except HipLibraryMissing:
        pytest.skip("library not built")
