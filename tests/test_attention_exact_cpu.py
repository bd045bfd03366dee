"""The exact-softmax yardstick of tests/test_attention_exact_gpu.py, tested without a GPU: the operands keep their promises, the
CPU emulation of the kernels' online softmax stays inside the componentwise bound, and three planted faults - each confined to one
query row - are rejected by that bound while the whole-tensor criteria the suite has used so far for the same format accept them."""
import numpy as np
import pytest
import torch

import _attention_exact as X

SHAPES = [(300, 530), (70, 4200)]
# (p_format, out_format, defer, shift, operand family): the fp8 kernels, the bf16 and the f16 builds of the 16-bit kernels
KERNELS = [("e4m3", "bf16", 3, 5, "fp8"), ("bf16", "bf16", 8, 0, "16bit"), ("f16", "f16", 8, 0, "16bit")]
KERNEL_IDS = ["fp8", "bf16", "f16"]


def test_scale_times_log2e_is_one_in_fp32():
    c = np.float32(X.LOG2E_F32)
    s = np.float32(X.SCALE)
    assert float(s) == X.SCALE and s * c == np.float32(1.0)
    below, above = np.nextafter(s, np.float32(0)), np.nextafter(s, np.float32(1))
    assert below * c == np.float32(1.0) - np.float32(2.0 ** -23) and above * c == np.float32(1.0) + np.float32(2.0 ** -23)
    assert float(torch.tensor(X.SCALE, dtype=torch.float32) * torch.tensor(X.LOG2E_F32, dtype=torch.float32)) == 1.0


@pytest.mark.parametrize("family", ["fp8", "16bit"])
@pytest.mark.parametrize("profile", X.PROFILES)
@pytest.mark.parametrize("sq,sk", SHAPES)
def test_operand_profiles_keep_their_conditions(sq, sk, profile, family):
    q, k, v = X.operands(2, 2, sq, sk, profile, seed=sq + sk, family=family)       # asserts `conditions` itself
    X.round_trips(q, k, v)
    assert set(q.unique().tolist()) <= {-1.0, 0.0, 1.0} and set(v.abs().unique().tolist()) == {1.0, 2.0, 3.0, 4.0}
    rest = torch.ones(X.D, dtype=torch.bool)
    rest[X.D_STAIR] = False
    assert set(k[..., rest].unique().tolist()) == {-1.0, 0.0, 1.0}
    assert bool((v.sign() == v.sign()[0, 0, :1]).all()), "one sign per channel"
    assert bool((q.abs().amax((0, 1, 2)) == 1).all()), "every head dim is used by some query row"
    stair = k[0, 0, :, X.D_STAIR]
    assert bool((k[..., X.D_STAIR] == stair).all())
    steps = (stair[1:] - stair[:-1])
    step = X.FAMILY[family]["step"] + 2           # the level rises by the family's step over the running max, 2 above the level
    if profile == "window":
        assert bool((stair == 0).all())
    elif profile == "stair_up":
        assert bool((steps >= 0).all()) and float(steps.max()) == step and int((steps == step).nonzero()[0]) > 0.9 * sk
    else:
        assert bool((stair[:64] == 0).all()) and bool((stair[64:] < 0).all()) and float(stair.min()) == -4
    facts = X.conditions(q, k, v, profile, family, 1, int((steps == step).nonzero()[0]) + 1 if profile == "stair_up" else None)
    print(f"{family} {profile} ({sq}, {sk}): {facts}")
    assert facts["flat_rows"] > 0
    # chunked streams cut their tiles per chunk: the same promises
    X.operands(1, 2, sq, sk - sk % 4, profile, seed=1, family=family, nchunks=4)


def test_one_tile_stream_has_no_stair():
    for profile in X.PROFILES:
        q, k, v = X.operands(5, 2, 49, 9, profile, seed=3)
        assert bool((k[..., X.D_STAIR] == 0).all())


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("profile", X.PROFILES)
@pytest.mark.parametrize("sq,sk", SHAPES)
def test_emulation_stays_inside_the_bound(sq, sk, profile, kernel):
    p_format, out_format, defer, shift, family = kernel
    q, k, v = X.operands(1, 2, sq, sk, profile, seed=sq + sk + 1, family=family)
    ref = X.reference(q, k, v)
    out = X.emulate(q, k, v, p_format, out_format, defer, shift)
    worst, _, _ = X.ratio(out, ref, X.bound(ref, sk, out_format), f"emulation {p_format}/{out_format} {profile} ({sq}, {sk})")
    assert bool(torch.isfinite(out).all()) and worst <= 1.0
    exact = X.emulate(q, k, v, p_format, out_format, 0, shift)          # re-based at every rise of the max
    assert X.ratio(exact, ref, X.bound(ref, sk, out_format), "  exact re-base")[0] <= 1.0


def _old_criterion(out, ref, p_format):
    """The whole-tensor criteria of tests/test_kernels_gpu.py::_attn_close (16-bit) and tests/test_attention_fp8.py (fp8)."""
    out, ref = out.double(), ref.double()
    rel = float((out - ref).norm() / ref.norm())
    mx = float((out - ref).abs().max())
    if p_format == "e4m3":
        return rel < 6e-2 and mx / float(ref.abs().max()) < 0.12, rel, mx / float(ref.abs().max())
    rms = float(ref.pow(2).mean().sqrt())
    return rel <= 1e-2 and mx <= 0.25 * rms, rel, mx / rms


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("fault", ["p_off", "l_miss", "alpha"])
def test_planted_faults_pass_the_old_criterion_and_fail_the_bound(fault, kernel):
    """Why this yardstick exists.  The 8 keys behind the step of a stair_up stream (400 keys for the fp8 step, 16000 for the
    16-bit one) carry 5 .. 7 % of their row each; the fault sits on the one that carries least."""
    p_format, out_format, defer, shift, family = kernel
    sq, sk = 300, {"fp8": 400, "16bit": 16000}[family]
    q, k, v = X.operands(1, 2, sq, sk, "stair_up", seed=7, family=family)
    ref = X.reference(q, k, v)
    bnd = X.bound(ref, sk, out_format)
    b, row, key, w = X.fault_site(q, k, v)
    assert sk - 10 <= key < sk and 0.05 <= w < 0.08
    good = X.emulate(q, k, v, p_format, out_format, defer, shift)
    assert X.ratio(good, ref, bnd, f"{p_format}/{out_format} fault-free")[0] <= 1.0
    bad = X.emulate(q, k, v, p_format, out_format, defer, shift, fault=fault)
    worst, wrow, _ = X.ratio(bad, ref, bnd, f"{p_format}/{out_format} fault {fault} on a key of weight {w:.3f}")
    ok_old, rel, mx = _old_criterion(bad, ref, p_format)
    print(f"  old criterion: rel-L2 {rel:.3e}, max-abs clause {mx:.3e} -> {'accepted' if ok_old else 'rejected'}")
    assert worst > 1.0 and wrow == row, "the componentwise bound must reject the fault, on the faulted row"
    assert ok_old, "the whole-tensor criterion accepts the same output"
    differs = ((bad - good).abs().amax(-1) > 0).nonzero().flatten().tolist()
    assert differs == [row], "the fault is confined to one query row"
