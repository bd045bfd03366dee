"""The exact-GEMM yardstick of tests/test_gemm_exact_gpu.py, tested without a GPU: the operands of every case keep their conditions,
a CPU emulation of the epilogue (fp32 torch, the kernels' rounding points) equals the reference whatever the order of its K sum, and
five faults planted at a rounding point pass the tolerance tests/test_kernels_gpu.py::test_gemm uses while the exact comparison
rejects each of them - as it rejects one dropped k-step."""
import math

import pytest
import torch

import _gemm_exact as X

NAMES = list(X.DTYPES)
IDS = [X.case_id(c) for c in X.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_conditions_hold_for_every_case(name):
    """Both files draw their cases from X.CASES.  Prints, per case, the shares of outputs that need rounding and of ties."""
    seen = set()
    for case in X.CASES:
        c, lin, want = X.operands(case, name)
        f = X.conditions(c)
        print(f"{name} {X.case_id(case)}: {f['outputs']} outputs, std {f['std']:.1f}, needs rounding {f['needs_rounding']:.3f}, ties {f['ties']:.3f} "
              f"(up {f['ties_up']:.3f}, down {f['ties_down']:.3f}), zeros {f['zeros']}" + (f", |lin| <= {f['max_abs']}, {f['beyond_table']} at |lin| >= 8" if c.gelu else ""))
        seen.add((case.kernel, case.epi))
    for kernel in ("k128", "pingpong", "tail"):
        assert {e for k, e in seen if k == kernel} == set(X.EPILOGUES), f"{kernel} misses an epilogue"
    assert {e for k, e in seen if k == "lockstep"} == {"plain", "bias", "bias_res", "res_inplace", "gelu"}


def test_case_table_reaches_what_it_names():
    """The dispatch arithmetic of am_gemm_bf16 restated: which cases split off remainder rows, and where they go."""
    for c in X.CASES:
        rem = c.M % 256
        split = rem != 0 and rem <= 128 and c.M > 2048
        big_auto = c.N >= 256 and c.M >= 1024 and -(-c.M // 256) * -(-c.N // 256) >= 192
        assert c.K % 64 == 0 and c.N % 8 == 0 and (c.k1 == 0 or (c.k1 % 64 == 0 and 0 < c.k1 < c.K))
        assert split == (c.kernel in ("tail", "tail128", "dispatch")), c
        assert big_auto == (c.kernel == "dispatch"), c
        if c.kernel == "tail":
            assert not c.a_map and not c.c_map and c.N % 4 == 0
        if c.kernel == "tail128":
            assert c.c_map
        if c.epi.startswith("fold"):
            assert c.kernel != "lockstep" and not c.k1 and (not c.a_map or c.kernel == "k128")
        for m in (c.a_map, c.c_map):
            assert not m or c.M % m[0] == 0
    assert len(X.CASES) <= 68


def test_rounding_helpers_agree_with_torch():
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(20000, generator=g) * 3000).float()
    for name in NAMES:
        assert torch.equal(X._round_with(x, name, "nearest_even"), x.to(X.DTYPES[name]).float())
        t, h, r = X._round_with(x, name, "truncate"), X._round_with(x, name, "half_away"), X._round_with(x, name, "nearest_even")
        for y in (t, h):
            assert torch.equal(y.to(X.DTYPES[name]).float(), y), "not a value of the type"
        assert bool((t.abs() <= x.abs()).all()) and bool(((t - x).abs() >= (r - x).abs()).all())
        assert bool(((h - x).abs() == (r - x).abs()).all()) and bool((h.abs() >= r.abs()).all())
    ties = torch.tensor([257.0, 259.0, -257.0, 2049.0, 2051.0])
    assert X._round_with(ties, "bf16", "nearest_even")[:3].tolist() == [256.0, 260.0, -256.0]
    assert X._round_with(ties, "bf16", "half_away")[:3].tolist() == [258.0, 260.0, -258.0]
    assert X._round_with(ties, "f16", "nearest_even")[3:].tolist() == [2048.0, 2052.0] and X._round_with(ties, "f16", "truncate")[3:].tolist() == [2048.0, 2050.0]
    f = X.rounding_facts(torch.tensor([257.0, 259.0, 256.0, 0.0, 513.0, 3.0]).double(), "bf16")
    assert (f["needs_rounding"], f["ties"], f["ties_up"], f["ties_down"], f["zeros"]) == (0.5, 2 / 6, 1 / 6, 1 / 6, 1)


@pytest.mark.parametrize("name", NAMES)
def test_emulation_equals_reference_in_every_k_order(name):
    """Ascending from zero, four descending K-quarters summed pairwise, ascending from the bias: the same bits, and the reference's."""
    for case in X.CASES:
        if case.epi.endswith("gelu"):
            continue
        c, lin, want = X.operands(case, name)
        for order in X.ORDERS:
            out = X.emulate(c, order)
            rep = X.mismatch_report(out, want, X.TILE[case.kernel], X.pre_rounding(c)[0], f"emulation {order} {name} {X.case_id(case)}", name)
            assert rep is None, rep


def _old_criterion(out, c):
    """tests/test_kernels_gpu.py::test_gemm restated: the fp32 statement, rounded once; |out - ref| <= 2 u max(|ref|, mag) + atol with
    atol = 2e-3 sqrt(K / 64) and mag = max(|lin|, |res|).  u is 2^-8 there (bf16); the f16 cases get f16's 2^-11, the stricter reading.
    Under a fold the statement is tests/test_ln_fold_gpu.py's: rstd (acc - mean colsum) + d."""
    a = (torch.cat([c.a, c.a2], 1) if c.a2 is not None else c.a)[c.aidx].float()
    ref = a @ c.w.float().T
    if c.fold:
        st = c.stats[c.aidx].float()
        ref = st[:, 1:] * (ref - st[:, :1] * c.colsum.float())
    if c.bias is not None:
        ref = ref + c.bias.float()
    ref = ref.to(X.DTYPES[c.name]).float()
    mag = ref.abs()
    if c.res is not None:
        res = c.res[c.cidx].float()
        mag = torch.maximum(mag, res.abs())
        ref = ref + res
    tol = 2.0 * X.U_OUT[c.name] * torch.maximum(ref.abs(), mag) + 2e-3 * math.sqrt(c.case.K / 64)
    bad = (out.float() - ref).abs() > tol
    return not bool(bad.any()), int(bad.sum())


# The tolerance of test_gemm has room for two half-spacings relative to the RESULT, so each fault is planted where it is the epilogue's
# only extra error: the faults of the linear's rounding on bias cases of the table, the residual fault on bias + residual cases.  A
# rounding in front of the shift (bias, or the fold's) errs by half a spacing of the ACCUMULATOR: where the shift pulls the result
# below the power of two the accumulator stands above, that is 2 u 2^k against a tolerance of 2 u |result| + atol, and |result| is up
# to |shift| short of 2^k.  test_gemm's bias (0.5 sigma against outputs of sigma 1) makes that rare; here it is made impossible:
# K = 1024 (atol 0.008) and operands(small_shift=True), |shift| <= 1 in bf16 (u = 2^-8) and 8 in f16 (2^-11): short by 0.0078 at most.
_BIAS = [X.Case("k128", 129, 136, 192, "bias"), X.Case("pingpong", 1300, 520, 1024, "bias"), X.Case("tail", 2048 + 32, 328, 576, "bias")]
_RES = [X.Case("k128", 300, 328, 1024, "bias_res"), X.Case("pingpong", 777, 328, 192, "bias_res"), X.Case("tail", 2048 + 33, 328, 1024, "bias_res")]
_SHIFT_BIAS = [X.Case("k128", 300, 328, 1024, "bias"), X.Case("pingpong", 1300, 520, 1024, "bias"), X.Case("tail", 2048 + 33, 328, 1024, "bias")]
_SHIFT_FOLD = [X.Case("k128", 300, 328, 1024, "fold"), X.Case("pingpong", 1300, 520, 1024, "fold"), X.Case("tail", 2048 + 128, 328, 1024, "fold")]
FAULT_CASES = {"residual_before_rounding": _RES, "bias_after_rounding": _SHIFT_BIAS, "fold_rounded_twice": _SHIFT_FOLD}


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("fault", X.FAULTS)
def test_planted_faults_pass_the_old_criterion_and_fail_the_exact_one(fault, name):
    for case in FAULT_CASES.get(fault, _BIAS):
        small = fault in ("bias_after_rounding", "fold_rounded_twice")
        assert small or case in X.CASES
        c, lin, want = X.operands(case, name, small_shift=small)
        X.conditions(c)
        good = X.emulate(c, "quarters")
        assert X.mismatch_report(good, want, X.TILE[case.kernel]) is None and _old_criterion(good, c)[0]
        bad = X.emulate(c, "quarters", fault=fault)
        rep = X.mismatch_report(bad, want, X.TILE[case.kernel], X.pre_rounding(c)[0], f"{fault} {name} {X.case_id(case)}", name)
        ok_old, n_old = _old_criterion(bad, c)
        print(f"{rep}\n  old criterion: {'accepted' if ok_old else f'rejected, {n_old} elements'}")
        assert rep is not None, "the exact comparison must reject the fault"
        share = float((bad.double() != want).sum()) / want.numel()
        if fault == "one_k_step_dropped":
            assert "row % " in rep and share <= 32 / case.M + 1e-9         # confined to the 32 rows that lost the step
        else:
            assert ok_old, f"the tolerance of test_gemm must accept {fault} ({n_old} elements outside)"
            assert share >= 0.02, f"{fault} moves only {share:.4f} of the outputs"
        if fault in ("truncate", "half_away"):
            assert rep.rstrip().endswith("True") == (fault == "half_away")   # half-away differs from nearest-even on ties alone


@pytest.mark.parametrize("name", NAMES)
def test_pre_shift_faults_fail_the_exact_comparison_on_the_table_operands(name):
    """bias_after_rounding and fold_rounded_twice above run on small_shift operands, for the old criterion's sake.  On the operands the
    GPU file runs (|bias| <= 32, 256 in f16) their effect is larger, and the exact comparison rejects them there too."""
    for fault, epis in (("bias_after_rounding", ("bias", "bias_res")), ("fold_rounded_twice", ("fold", "fold_d", "fold_d_res"))):
        cases = [c for c in X.CASES if c.epi in epis and c.M * c.N <= 2 ** 20]
        assert {c.kernel for c in cases} >= {"k128", "pingpong", "tail"} - ({"lockstep"} if fault == "fold_rounded_twice" else set())
        for case in cases:
            c, lin, want = X.operands(case, name)
            bad = X.emulate(c, "ascending", fault=fault)
            share = float((bad.double() != want).sum()) / want.numel()
            print(f"{fault} {name} {X.case_id(case)}: {share:.4f} of the outputs differ")
            assert share >= 0.02, f"{fault} on {X.case_id(case)} moves only {share:.4f} of the outputs"


def test_tail_kernel_meets_every_epilogue_at_both_edges():
    """Each of the nine epilogues reaches gemm_tail_kernel with a partial 32-row block (r = 1 or 33) and with the 8-column last block
    (N = 328); every r, N and K of the issue's table appears."""
    tail = [c for c in X.CASES if c.kernel == "tail"]
    for e in X.EPILOGUES:
        assert any(c.epi == e and (c.M - 2048) % 32 for c in tail), f"{e}: no partial row block"
        assert any(c.epi == e and c.N % 64 for c in tail), f"{e}: no partial column block"
    assert {c.M - 2048 for c in tail} == {1, 32, 33, 128} and {c.N for c in tail} == {64, 328} and {c.K for c in tail} == {64, 576, 1024}
    assert any(c.k1 == 192 and c.K == 576 for c in tail)


def test_mismatch_report_names_the_place():
    want = torch.arange(512 * 256, dtype=torch.float64).view(512, 256)
    assert X.mismatch_report(want.clone(), want, (128, 128)) is None
    out = want.clone()
    out[130, 7] += 1
    out[386, 135] = float("nan")
    rep = X.mismatch_report(out, want, (128, 128), want, "case", "bf16")
    assert "2 of 131072" in rep and "(130, 7): got 33288.0, want 33287.0, exact 33287.0" in rep and "row % 128: [2]" in rep and "col % 128: [7]" in rep
    z = torch.zeros(2, 2, dtype=torch.float64)
    assert X.mismatch_report(-z, z, (128, 128)) is None                     # +0 == -0
    inf = torch.full((2, 2), float("inf"), dtype=torch.float64)
    assert X.mismatch_report(inf, inf, (128, 128)) is not None              # equal, but not finite


def test_gelu_bound_is_the_stated_one():
    lin = torch.tensor([[-9.0, -1.0, 0.0, 0.125, 3.0, 12.0]], dtype=torch.float64)
    g = X.gelu_fp64(lin)
    assert torch.allclose(g, torch.nn.functional.gelu(lin), rtol=0, atol=1e-15) and float(g[0, 0]) < 0 and float(g[0, 5]) == 12.0
    for name in NAMES:
        worst, rep = X.gelu_check(X.rnd(g, name), lin, name)
        assert rep is None and worst <= 1.0
        off = g * (1 + 2.5 * X.U_OUT[name])
        worst, rep = X.gelu_check(off, lin, name)
        assert rep is not None and worst > 1.0
    assert X.GELU_E == 3.3e-7
