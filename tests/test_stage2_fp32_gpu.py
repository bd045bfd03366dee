"""Exact-fp32 Stage II on the device (GPU): am_rope_f32 (csrc/am_stage1_f32.hip) against its contract in include/actionmesh_amd.h,
HipAutoencoder(exact_fp32=True) on the fixtures and on the cases they do not reach (the assertions of tests/test_stage2_fp32_cpu.py, now
on the kernels), and the use the mode is for: standing in for the reference's host fp32 forward as the yardstick of a 16-bit run.

Bounds.  am_rope_f32: the bits of oracle.denoiser_oracle.apply_rope evaluated on the CPU as separate torch fp32 operations - two
products and a sum per element, each rounded once.  Model level: rel-L2 <= 2e-5 against the reference's own fp32 displacement
(tests/_stage2_fp32.py).  The yardstick test is the triangle inequality: no number is chosen."""
import math

import pytest
import torch

import _stage2_fp32 as S
from _guard import Arena

pytestmark = pytest.mark.gpu
HD = 128


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from actionmesh_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---- am_rope_f32 -----------------------------------------------------------------------------------------------------------------
def _tables(frames):
    from actionmesh_amd.denoiser import rope_tables_host
    return rope_tables_host(torch.arange(frames, dtype=torch.float32)[None] * 1.5 + 2.0)        # (frames, 64) each


def _rope_reference(x, heads, offs, hs, cos, sin, rpf):
    """The contract through the oracle's apply_rope on the CPU: (expected, mask of the addressed chunks)."""
    from oracle.denoiser_oracle import apply_rope
    rows = x.shape[0]
    frame = torch.arange(rows) // rpf
    cs, sn = (t[frame].repeat_interleave(2, dim=1)[None] for t in (cos, sin))                   # (1, rows, 128)
    want, chunk = x.clone(), torch.zeros_like(x, dtype=torch.bool)
    for off in offs:
        cols = [slice(off + h * hs, off + h * hs + HD) for h in range(heads)]
        xh = torch.stack([x[:, c] for c in cols], 0)[None]                                      # (1, H, rows, 128)
        out = apply_rope(xh, cs, sn)[0]
        for h, c in enumerate(cols):
            want[:, c] = out[h]
            chunk[:, c] = True
    return want, chunk


def _assert_same_bits_or_nan(got, want, what):
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN positions differ"
    same = got.view(torch.int32)[~nan] == want.view(torch.int32)[~nan]
    assert bool(same.all()), f"{what}: {int((~same).sum())} element(s) differ, max |difference| {float((got[~nan] - want[~nan]).abs().max())}"


SPECIALS = [0.0, -0.0, 1e-40, -3e-42, float("inf"), float("-inf"), float("nan"), 3.0e38, -3.0e38]


@pytest.mark.parametrize("kinds", [1, 2])
@pytest.mark.parametrize("rows,heads", [(1, 1), (7, 2), (9, 8), (1031, 8), (1, 4), (3, 3)])
def test_rope_f32_is_the_torch_fp32_expression(dev, rows, heads, kinds):
    """Bit for bit, every element: the packed [q | k | v] per head layout (head stride 3 hd; one kind: the k chunks alone; two kinds: q
    and k in ONE launch), rows_per_frame of 1, 5 and 257 with the last frame partial, a row stride equal to the packed width and one
    4 floats wider, +-0, denormals, +-inf, huge values and NaN scattered over the chunks.  Chunk counts rows x heads x kinds of 1, 2, 4,
    8, 9, 14, 18, 28, 72, 144 and 8248 / 16496 lie on both sides of the 8 chunks of a workgroup.  X sits in a poisoned arena (the gap behind a
    padded row and the guard rows are sentinels), the tables in arenas of their own; the v chunks keep their bits."""
    from actionmesh_amd import ops
    gen = torch.Generator().manual_seed(rows * 31 + heads * 7 + kinds)
    width, hs = 3 * HD * heads, 3 * HD
    offs = (HD,) if kinds == 1 else (0, HD)
    for rpf in (1, 5, 257):
        frames = (rows + rpf - 1) // rpf
        for pad in (0, 4):
            x = torch.randn((rows, width), generator=gen) * 3.0
            pos = torch.randint(0, rows * width, (min(rows * width // 8, 4096),), generator=gen)
            x.view(-1)[pos] = torch.tensor(SPECIALS)[torch.arange(pos.numel()) % len(SPECIALS)]
            cos, sin = _tables(frames)
            want, chunk = _rope_reference(x, heads, offs, hs, cos, sin, rpf)
            X = Arena.of(x.to(dev), ld=width + pad)
            Cs, Sn = Arena.flat_of(cos.to(dev)), Arena.flat_of(sin.to(dev))
            ops.rope_f32(X.view, heads, (Cs.view, Sn.view), off_a=offs[0], off_b=-1 if kinds == 1 else offs[1], head_stride=hs,
                         rows_per_frame=rpf)
            torch.cuda.synchronize()
            what = f"rows={rows} heads={heads} kinds={kinds} rows_per_frame={rpf} pad={pad}"
            X.assert_untouched("X " + what)
            Cs.assert_untouched("cos"); Sn.assert_untouched("sin")
            assert torch.equal(Cs.view.cpu(), cos) and torch.equal(Sn.view.cpu(), sin)
            got = X.view.cpu()
            assert torch.equal(got[~chunk].view(torch.int32), x[~chunk].view(torch.int32)), f"{what}: a column outside the addressed chunks changed"
            _assert_same_bits_or_nan(got, want, what)


def test_rope_f32_both_library_builds_give_the_same_bits(dev):
    from actionmesh_amd import ops
    gen = torch.Generator().manual_seed(3)
    x = torch.randn((10, 3 * HD * 2), generator=gen).to(dev)
    cos, sin = (t.to(dev) for t in _tables(2))
    a = ops.rope_f32(x.clone(), 2, (cos, sin), off_a=0, off_b=HD, head_stride=3 * HD, rows_per_frame=5, kind="bf16")
    b = ops.rope_f32(x.clone(), 2, (cos, sin), off_a=0, off_b=HD, head_stride=3 * HD, rows_per_frame=5, kind="f16")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and not torch.equal(a, x)
    assert torch.equal(a[:, 2 * HD:3 * HD], x[:, 2 * HD:3 * HD])                  # the v chunks


def test_rope_f32_refuses_what_it_cannot_address(dev):
    """Every refusal comes from the library (the wrapper's own checks are bypassed), reports through am_last_error, launches nothing
    and writes nothing: X keeps its bits."""
    from actionmesh_amd import ops
    heads, hs, width = 2, 3 * HD, 3 * HD * 2
    x0 = torch.randn((4, width + hs), generator=torch.Generator().manual_seed(1))       # rows of 9 hd: room for a third head's chunks
    x = x0.to(dev)
    cos, sin = (t.to(dev) for t in _tables(2))
    X, Cp, Sp, ld = x.data_ptr(), cos.data_ptr(), sin.data_ptr(), x.stride(0)

    def refused(match, *args):
        with pytest.raises(RuntimeError, match=match):
            ops._call(x, "bf16", "am_rope_f32", *args)

    #                  X      ldx  off_a off_b  hs     rows heads cos  sin  frames rows_per_frame
    refused("null", None, ld, 0, HD, hs, 4, heads, Cp, Sp, 2, 2)
    refused("null", X, ld, 0, HD, hs, 4, heads, None, None, 2, 2)
    refused("pairs", X, ld, 0, HD, hs, 4, heads, Cp, None, 2, 2)                   # one table without the other
    refused("pairs", X, ld, 0, HD, hs, 4, heads, None, Sp, 2, 2)
    refused("aligned", X + 4, ld, 0, HD, hs, 4, heads, Cp, Sp, 2, 2)                # X off a 16-byte boundary
    refused("aligned", X, ld - 2, 0, HD, hs, 4, heads, Cp, Sp, 2, 2)                # ldx
    refused("aligned", X, ld, 2, HD, hs, 4, heads, Cp, Sp, 2, 2)                    # off_a
    refused("aligned", X, ld, 0, HD + 2, hs, 4, heads, Cp, Sp, 2, 2)                # off_b
    refused("aligned", X, ld, 0, HD, hs + 2, 4, heads, Cp, Sp, 2, 2)                # head_stride
    refused("overlap", X, ld, 0, 64, hs, 4, heads, Cp, Sp, 2, 2)                    # k chunk of head h half inside its q chunk
    refused("overlap", X, ld, 0, 0, hs, 4, heads, Cp, Sp, 2, 2)                     # the same chunks twice
    refused("overlap", X, ld, 64, hs, hs, 4, heads, Cp, Sp, 2, 2)                   # k chunk of head 0 inside the q chunk of head 1
    refused("overlap", X, ld, 0, HD, 64, 4, heads, Cp, Sp, 2, 2)                    # heads of one kind overlap each other
    refused("past the row", X, width + 8, 0, 2 * HD + 16, hs, 4, heads, Cp, Sp, 2, 2)      # the last k chunk ends behind ldx
    refused("past the row", X, 2 * HD, 0, -1, hs, 4, heads, Cp, Sp, 2, 2)           # one kind: head 1 ends behind ldx
    refused("frames", X, ld, 0, HD, hs, 4, heads, Cp, Sp, 1, 3)                     # row 3 is frame 1, the tables hold one
    refused("frames", X, ld, 0, HD, hs, 4, heads, Cp, Sp, 2, 0)
    refused("bad shape", X, ld, 0, HD, hs, 0, heads, Cp, Sp, 2, 2)
    torch.cuda.synchronize()
    assert torch.equal(x.cpu().view(torch.int32), x0.view(torch.int32))
    with pytest.raises(ValueError, match="columns"):                                # ... and what the wrapper itself sees first
        ops.rope_f32(x[:, :width], 3, (cos, sin), off_a=0, off_b=HD, head_stride=hs)
    with pytest.raises(ValueError, match="frames"):
        ops.rope_f32(x[:, :width], 2, (cos, sin), off_a=0, off_b=HD, head_stride=hs, rows_per_frame=1)
    ops.rope_f32(x[:, :width], heads, (cos, sin), off_a=0, off_b=HD, head_stride=hs, rows_per_frame=2)      # the same call, well formed
    assert not torch.equal(x.cpu(), x0) and torch.equal(x.cpu()[:, width:], x0[:, width:])


# ---- the model on the fixtures -------------------------------------------------------------------------------------------------------
MODES_16 = [(dt, kw) for dt in ("bfloat16", "float16") for kw in (dict(residual_fp32=False), dict(), dict(cross_fp32=True))]


@pytest.fixture(scope="module", params=["ae_tiny", "ae_arch"])
def fixture_runs(request, dev, golden_dir):
    """One fixture's exact forward and its six 16-bit forwards (bf16 and float16, each with residual_fp32=False, the default, and
    cross_fp32=True): computed once, shared by the tests below.  ae_arch is the shipped architecture at 8 x 256 tokens, 2000 vertices,
    3 targets."""
    name = request.param
    model, cfg, sd, t, d32, r32 = S.check_fixture(name, golden_dir, dev)
    counts = model.entry_counts()
    low = {}
    for dt, kw in MODES_16:
        m = S.build(cfg, sd, dev, exact_fp32=False, dtype=dt, **kw)
        low[(dt, ", ".join(f"{k}={v}" for k, v in kw.items()) or "default")] = S.run(m, t, dev)
        m.to("cpu")
    return dict(name=name, model=model, cfg=cfg, t=t, d32=d32, r32=r32, low=low, counts=counts)


def test_forward_against_the_reference_fp32_displacement(fixture_runs):
    """seen on MI355X: ae_tiny 6.61e-7 (max abs 1.07e-6), ae_arch 1.49e-6 (max abs 2.09e-6); profiles/stage2_fp32.json, DESIGN section 6 N15"""
    f = fixture_runs
    assert f["r32"] <= S.BOUND
    B, T_out = f["t"]["target_alphas"].shape
    assert f["counts"] == S.expected_counts(f["cfg"].num_layers, T_out, B), f["counts"]


def test_exact_mode_is_closer_to_the_reference_than_every_16_bit_mode(fixture_runs):
    f = fixture_runs
    ref = f["t"]["displacement_fp32"]
    for key, d in f["low"].items():
        r = S.rel(d, ref)
        print(f"{f['name']}: {key[0]} ({key[1]}) rel-L2 vs the reference's fp32 displacement {r:.3e} (exact mode {f['r32']:.3e})")
        assert d.dtype == torch.float32 and f["r32"] < r, (key, f["r32"], r)


def test_device_fp32_stands_in_for_the_host_fp32_forward(fixture_runs):
    """The yardstick in use: the bf16 default run's distance to the DEVICE fp32 run and to the fixture differ by no more than the
    device-to-fixture distance - the triangle inequality, all three measured with the fixture's norm."""
    f = fixture_runs
    ref, d32, b = f["t"]["displacement_fp32"].double(), f["d32"].double(), f["low"][("bfloat16", "default")].double()
    n = float(ref.norm())
    r_dev, r_fix, gap = float((b - d32).norm()) / n, float((b - ref).norm()) / n, float((d32 - ref).norm()) / n
    print(f"{f['name']}: bf16 default vs the device fp32 run {r_dev:.4e}, vs the reference's fp32 displacement {r_fix:.4e}, "
          f"device fp32 vs the reference {gap:.3e}")
    assert abs(r_dev - r_fix) <= gap * (1 + 1e-9) and gap <= S.BOUND


# ---- the cases the fixtures do not reach, state between targets, the window loop ----------------------------------------------------------
@pytest.mark.parametrize("case", S.CASES, ids=[c[0] for c in S.CASES])
def test_cases_the_fixtures_do_not_reach(dev, case):
    S.check_case(case, dev)


def test_no_state_leaks_between_targets(dev):
    S.check_no_state_between_targets(dev)


def test_vertex_animation_passes_the_exact_mode_through(dev):
    S.check_vertex_animation(dev)


# ---- it really is fp32 --------------------------------------------------------------------------------------------------------------------
def test_only_f32_entry_points_run_and_autocast_changes_nothing(dev, golden_dir, monkeypatch):
    """Every entry point the library is asked for during an exact forward is recorded at ops._entry, the one door to it: only the six
    fp32 ones, no 16-bit GEMM, attention or layernorm.  The reference pipeline calls Stage II inside torch.autocast("cuda", dtype)
    (pipeline.py:679): a 16-bit model takes its type from the region, the exact model computes the same bits inside it as outside."""
    from actionmesh_amd import ops
    cfg, sd, t = S.fixture(golden_dir, "ae_tiny")
    model = S.build(cfg, sd, dev)
    asked, entry = [], ops._entry

    def recording_entry(key, name):
        asked.append(name)
        return entry(key, name)
    monkeypatch.setattr(ops, "_entry", recording_entry)
    d = S.run(model, t, dev)
    assert set(asked) == S.F32_ENTRIES, set(asked)
    assert len(asked) == sum(model.entry_counts().values())
    assert model._w_kind == {}                                                    # no 16-bit weights were uploaded
    asked.clear()
    with torch.autocast("cuda", dtype=torch.float16):
        assert model.compute_kind() == "f32"
        da = S.run(model, t, dev)
    assert set(asked) == S.F32_ENTRIES and da.dtype == torch.float32
    assert torch.equal(da.view(torch.int32), d.view(torch.int32))
    assert math.isfinite(float(d.abs().max()))
