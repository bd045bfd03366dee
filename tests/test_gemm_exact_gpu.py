"""Every GEMM kernel behind am_gemm_bf16, bit for bit, on exactly summable operands (GPU), in both 16-bit builds.

tests/_gemm_exact.py: integer operands times one power of two, sum |a||w| + |bias| below 2^24 quanta - every fp32 partial sum is exact
in any order, MFMA shape and K split, so each output has one correct bit pattern: rnd(exact + bias) (or the folded LayerNorm's two
exact FMAs), then rnd(lin + residual).  A differing element is a defect of the kernel; the assertion names its tile residues and says
whether the mismatches are ties.  GELU cases compare with gelu_fp64 of the exactly known pre-activation within u |g| + (1 + u) E, E the
error am_common.h states for gelu_erf.  The table of cases (kernel x shape x epilogue) is X.CASES; tests/test_gemm_exact_cpu.py checks
the operands' conditions for every one of them and that the comparison rejects misplaced roundings the tolerance tests accept."""
import os

import pytest
import torch

import _gemm_exact as X

pytestmark = pytest.mark.gpu

SWITCHES = {"k128": dict(force_small=True), "lockstep": dict(force_big=True, legacy=True), "pingpong": dict(force_big=True), "dispatch": {},
            "tail": dict(force_big=True), "tail128": dict(force_big=True)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from actionmesh_amd import _lib
    _lib.lib()   # fail loudly if the HIP library is missing
    _lib.lib("f16")
    # which kernel a case reaches also hangs on the library's A/B switches: with one of them set the table would name another kernel
    for var in ("ACTIONMESH_AMD_GEMM_TAIL", "ACTIONMESH_AMD_GELU_TABLE", "ACTIONMESH_AMD_GEMM_SKEW"):
        assert var not in os.environ, f"{var} is set: the cases of tests/_gemm_exact.py would not reach the kernels they name"
    yield torch.device("cuda:0")
    X._a_w.cache_clear()          # the shared operands go with the module


def _run(c, dev):
    """ops.gemm on the built case -> the logical rows of the output, on the CPU.  Asserts that the rows a c_map skips still hold what
    they held before (the sentinel, or the residual they alias)."""
    from actionmesh_amd import _lib as L
    from actionmesh_amd import ops
    case, dt = c.case, X.DTYPES[c.name]

    def dv(t, d=dt):
        return None if t is None else t.to(d).to(dev).contiguous()

    res = dv(c.res)
    if case.epi == "res_inplace":
        out = res.clone()
        residual = out                                    # out is residual
    else:
        out = torch.full((c.rows_c, case.N), X.SENTINEL, dtype=dt, device=dev) if case.c_map else None
        residual = res
    before = out.clone().cpu() if out is not None else None
    kw = dict(SWITCHES[case.kernel])
    if c.fold:
        kw["ln"] = (dv(c.stats, torch.float32), dv(c.colsum, torch.float32))
    out = ops.gemm(dv(c.a), dv(c.w), bias=dv(c.bias, torch.float32), residual=residual, gelu=c.gelu, a2=dv(c.a2), out=out,
                   a_map=case.a_map or (0, 0, 0), c_map=case.c_map or (0, 0, 0), M=case.M, ablate=case.skew << L.GEMM_SKEW_SHIFT, **kw)
    torch.cuda.synchronize()
    assert out.dtype == dt and tuple(out.shape) == (c.rows_c, case.N)
    out = out.cpu()
    skipped = torch.ones(c.rows_c, dtype=torch.bool)
    skipped[c.cidx] = False
    if case.c_map:
        assert int(skipped.sum()) == c.rows_c - case.M > 0
        assert torch.equal(out[skipped].view(torch.int16), before[skipped].view(torch.int16)), "a row the c_map skips was written"
    return out[c.cidx]


@pytest.mark.parametrize("case", X.CASES, ids=[X.case_id(c) for c in X.CASES])
@pytest.mark.parametrize("name", list(X.DTYPES))
def test_gemm_is_exact(dev, name, case):
    c, lin, want = X.operands(case, name)
    X.conditions(c)                # on this machine's draw of the operands, before the kernel sees them
    got = _run(c, dev)
    what = f"{name} {X.case_id(case)}"
    if c.gelu:
        assert bool(torch.isfinite(got.float()).all()), f"{what}: output not finite"
        worst, rep = X.gelu_check(got, lin, name, what)
        assert rep is None, rep
        zero = lin == 0
        assert bool((got.double()[zero] == 0).all()), f"{what}: gelu(0) != 0"
    else:
        rep = X.mismatch_report(got, want, X.TILE[case.kernel], X.pre_rounding(c)[0], what, name)
        assert rep is None, rep


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("M,N,K", [(1, 8, 64), (37, 136, 96), (300, 328, 1024)])
def test_gemm_f32_is_exact(dev, M, N, K, kind):
    """am_gemm_f32 on integer-valued fp32 operands with every partial sum below 2^24: nothing is rounded anywhere, so the output is the
    int64 result - pure indexing and accumulation.  Epilogues: bias, residual, residual aliasing the output."""
    from actionmesh_amd import ops
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randint(-8, 9, (M, K), generator=g)
    w = torch.randint(-8, 9, (N, K), generator=g)
    bias = torch.randint(-1000, 1001, (N,), generator=g)
    res = torch.randint(-100000, 100001, (M, N), generator=g)
    a[torch.arange(M) % 37 == 5] = 0
    bias[::29] = 0
    assert int((a.abs() @ w.abs().T + bias.abs() + res.abs()).max()) < 2 ** 24
    lin = a @ w.T
    af, wf, bf, rf = (t.float().to(dev) for t in (a, w, bias, res))
    for what, kw, want in (("bias", dict(bias=bf), lin + bias), ("residual", dict(residual=rf), lin + res),
                           ("bias + residual", dict(bias=bf, residual=rf), lin + bias + res)):
        out = ops.gemm_f32(af, wf, kind=kind, **kw)
        torch.cuda.synchronize()
        rep = X.mismatch_report(out, want, (128, 128), want, f"gemm_f32 {kind} ({M}, {N}, {K}) {what}")
        assert rep is None, rep
    h = rf.clone()
    out = ops.gemm_f32(af, wf, bias=bf, residual=h, out=h, kind=kind)
    torch.cuda.synchronize()
    assert out is h
    rep = X.mismatch_report(h, lin + bias + res, (128, 128), lin, f"gemm_f32 {kind} ({M}, {N}, {K}) aliasing residual")
    assert rep is None, rep
