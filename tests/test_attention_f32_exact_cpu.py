"""tests/_attention_f32_exact.py without a GPU: the operands keep their promises for every case of the table, the CPU emulation of
attention_f32_kernel meets every expectation (bit for bit where bits are claimed, within the counted bound for `ladder`), and the
comparison rejects defects planted in the emulation - next to what the tolerance of tests/test_fp32_path_gpu.py (rel-L2 <= 2e-6 on
randn operands) makes of the same defect."""
import pytest
import torch

import _attention_f32_exact as X

OPERAND_SETS = sorted({(c.profile, c.shape, c.D, c.scale) for c in X.CASES}, key=str)
# every (profile, shape, head dim, scale) in the plain layout, every layout at the shape that has them all, the plateau in each
EMULATED = [c for c in X.CASES if c.layout == "plain" or c.shape == (2, 3, 97, 97) or c.profile == "plateau" and c.scale is None]
RANDN_BOUND = 2e-6                     # test_fp32_path_gpu.py::test_attention_f32_against_fp64


def _set_id(s):
    return X.case_id(X.Case(s[0], s[1], s[2], "", s[3]))


def _emulate(case, defect=None):
    q, k, v, info = X.operands(case.profile, case.shape, case.D, case.scale)
    mem = X.conditions(q, k, v, info)
    want = X.expected(q, k, v, info, mem)
    q2, k2, v2, kw = X.place(q, k, v, case.layout, lambda t: t)
    _, H, sq, sk = case.shape
    out = X.emulate(q2, k2, v2, H, sq, sk, case.D, scale=case.scale, defect=defect, **kw)
    return out, want, info, mem


def _verdict(case, out, want, info, mem):
    """None when `out` passes the check the GPU test makes of this case, else the text of its assertion."""
    what = X.case_id(case)
    if case.profile == "ladder":
        worst = X.ladder_ratio(out, want, -(-case.shape[3] // X.AK), what)
        return None if worst <= 1.0 else f"{what}: {worst:.3g} x the counted bound"
    return X.mismatch_report(out, want, info, mem, what)


def test_the_table_of_cases_is_complete():
    assert set(X.SHAPES) == {(1, 1, 1, 1), (2, 3, 33, 31), (2, 3, 129, 33), (1, 2, 300, 97), (3, 2, 65, 257), (2, 3, 97, 97)}
    assert X.PLATEAU_SHAPE == (1, 1, 128, 4113) and X.HEAD_DIMS == (64, 128) and X.SCALES == (1.0, 0.125, None)
    for prof in X.PROFILES:
        for D in X.HEAD_DIMS:
            shapes = {c.shape for c in X.CASES if c.profile == prof and c.D == D}
            assert shapes == ({X.PLATEAU_SHAPE} if prof == "plateau" else set(X.SHAPES)), (prof, D)
            for shape in shapes:
                lay = {c.layout for c in X.CASES if (c.profile, c.D, c.shape) == (prof, D, shape)}
                assert {"plain", "cross", "wide"} <= lay and ("packed" in lay) == (shape[2] == shape[3] and prof != "plateau")
                sc = {c.scale for c in X.CASES if (c.profile, c.D, c.shape) == (prof, D, shape)}
                assert sc == ({1.0} if prof == "ladder" else set(X.SCALES))
    assert len(set(X.CASES)) == len(X.CASES)
    assert X.ladder_bound(9) <= 1e-5


def test_the_two_facts_about_expf_hold_on_the_host():
    x = torch.tensor([0.0, -0.0, -104.0, -110.0, -1e30, float("-inf")])
    assert X._expf(x).tolist() == [1.0, 1.0, 0.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("oset", OPERAND_SETS, ids=[_set_id(s) for s in OPERAND_SETS])
def test_operands_keep_their_promises(oset):
    profile, shape, D, scale = oset
    q, k, v, info = X.operands(profile, shape, D, scale)
    mem = X.conditions(q, k, v, info)
    assert info["G"] * info["scale"] >= 110.0
    want = X.expected(q, k, v, info, mem)
    assert bool(torch.isfinite(want).all()) and float(want.abs().min()) > 0


@pytest.mark.parametrize("case", EMULATED, ids=[X.case_id(c) for c in EMULATED])
def test_emulation_meets_the_expectation(case):
    out, want, info, mem = _emulate(case)
    rep = _verdict(case, out, want, info, mem)
    assert rep is None, rep


def test_emulation_reads_only_what_the_layout_owns():
    """Every column no head owns is NaN in `place`'s layouts; the arithmetic above would carry one into the output."""
    for layout in X.LAYOUTS:
        case = X.Case("one_hot", (2, 3, 97, 97), 64, layout, None)
        out, *_ = _emulate(case)
        assert bool(torch.isfinite(out).all()), layout


# ---- planted defects -------------------------------------------------------------------------------------------------------------------
WITNESSES = [X.Case(p, s, 64, lay, None) for p, s, lay in (
    ("one_hot", (3, 2, 65, 257), "plain"), ("one_hot", (2, 3, 97, 97), "mixed"), ("subset", (2, 3, 97, 97), "cross"),
    ("order_rising", (3, 2, 65, 257), "plain"), ("order_first", (2, 3, 129, 33), "wide"))]
WITNESSES += [X.Case("ladder", (3, 2, 65, 257), 64, "plain", 1.0), X.Case("plateau", X.PLATEAU_SHAPE, 128, "plain", None)]
ONLY_HERE = {"ms_init_finite", "alpha_ulp_every_fourth_block", "v_head_stride_from_k"}      # the randn bound accepts these
BLIND = {"alpha_unrounded_max"}        # _attention_f32_exact's docstring: what the construction cannot see, and why


@pytest.fixture(scope="module")
def randn_case():
    """test_attention_f32_against_fp64's (1, 8, 300, 4113), D = 128 case cut to one head and 32 queries (the statistic is per row)."""
    g = torch.Generator().manual_seed(1000 + 300 + 4113 + 128)
    q, k, v = (torch.randn((n, 128), generator=g) for n in (32, 4113, 4113))
    ref = torch.softmax((q.double() @ k.double().T) * 128 ** -0.5, -1) @ v.double()
    return q, k, v, ref


def _randn_rel(randn_case, defect):
    q, k, v, ref = randn_case
    out = X.emulate(q, k, v, 1, 32, 4113, 128, defect=defect)
    return float((out.double() - ref).norm() / ref.norm())


def test_clean_emulation_on_the_randn_case(randn_case):
    rel = _randn_rel(randn_case, None)
    print(f"clean emulation on randn (1, 1, 32, 4113) D=128: rel-L2 {rel:.3e} (bound {RANDN_BOUND:.0e})")
    assert rel <= RANDN_BOUND


@pytest.mark.parametrize("defect", X.DEFECTS)
def test_planted_defect_is_rejected(defect, randn_case):
    """The defect, planted in the emulation, fails the comparison of at least one witness case; printed next to it, its rel-L2 on the
    randn case and whether the 2e-6 bound accepts it.
    seen, rel-L2 on randn against the 2e-6 bound (the clean emulation: 2.9e-7), and the witnesses that reject the defect here:
      alpha_unrounded_max           2.4e-6 rejected there; none here (BLIND: the helper's docstring says why)
      ms_init_finite                2.9e-7 ACCEPTED (no randn score comes near -87); one_hot, whose junk is up to 2^100 times its member
      alpha_ulp_every_fourth_block  1.1e-6 ACCEPTED; one_hot, subset, plateau
      v_head_stride_from_k          2.9e-7 ACCEPTED (no layout there has k_hs != v_hs); one_hot in the `mixed` layout
      tail_mask_off_by_one 1.5e-4, kvalid_previous_block 2.2e-3, bs_exchange_omitted 4.2e-3, rescale_judged_per_half 4.3e-1,
      v_row_swapped_halves 1.1     rejected there as well; here by 5 to 7 of the 7 witnesses
    ONLY_HERE is asserted: the 2e-6 bound accepts those three."""
    failed = []
    for case in WITNESSES:
        out, want, info, mem = _emulate(case, defect)
        rep = _verdict(case, out, want, info, mem)
        if rep is not None:
            failed.append(X.case_id(case))
    rel = _randn_rel(randn_case, defect)
    accepted = rel <= RANDN_BOUND
    print(f"{defect}: rel-L2 on randn {rel:.3e} (bound {RANDN_BOUND:.0e}: {'ACCEPTED' if accepted else 'rejected'}); "
          f"rejected here by {len(failed)} of {len(WITNESSES)} witnesses: {failed}")
    if defect in BLIND:
        assert not failed, f"{defect} is visible after all: take it out of BLIND and out of the helper's docstring: {failed}"
        assert rel > RANDN_BOUND, f"{defect} is guarded by neither comparison: rel-L2 {rel:.3e}"
    else:
        assert failed, f"{defect} passes every witness case"
    assert accepted == (defect in ONLY_HERE), f"{defect}: rel-L2 {rel:.3e} against {RANDN_BOUND:.0e}"
