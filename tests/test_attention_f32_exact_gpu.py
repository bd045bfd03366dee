"""am_attention_f32 per element on operands with one correct answer (GPU), through ops.attention_f32, in both library builds.

tests/_attention_f32_exact.py: integer Q and K whose member keys score exactly 0 and whose other keys score <= -110 / scale, so every
probability is expf(0) = 1 or expf(<= -110) = 0, the row sum is the member count, the numerator an exact sum, and the output one
correctly rounded division: `one_hot` returns the member's V row bit for bit (V is arbitrary fp32), `subset` / `order_*` / `plateau`
the correctly rounded mean of the members' integer V rows, `ladder` (the one profile with 0 < alpha < 1) stays within a bound counted
on the kernel's source.  X.CASES is profile x shape x head dim x layout x scale; tests/test_attention_f32_exact_cpu.py checks the
operands' promises for every case, that a CPU emulation of the kernel meets each expectation, and which planted defects fail it.

Every operand and the output stand in guard-band arenas (tests/_guard.py) with gaps behind the rows, every column no head owns is NaN,
and the neighbouring sequences hold member codes: a read or a write outside the logical operands changes a bit or a sentinel.
Measured on MI355X, both builds: every BITWISE case bit for bit - the division included, at every member count, so hipcc's fp32
division is the correctly rounded one here; `ladder` at most 0.071 of its bound."""
import functools

import pytest
import torch

import _attention_f32_exact as X
from _guard import SENTINEL, Arena

pytestmark = pytest.mark.gpu

KINDS = ("bf16", "f16")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from actionmesh_amd import _lib
    _lib.lib()   # fail loudly if the HIP library is missing
    _lib.lib("f16")
    yield torch.device("cuda:0")
    _answer.cache_clear()


@functools.lru_cache(maxsize=2)
def _answer(profile, shape, D, scale):
    """The operands, checked, and the expectation: once per (profile, shape, head dim, scale), shared by the layouts."""
    q, k, v, info = X.operands(profile, shape, D, scale)
    mem = X.conditions(q, k, v, info)      # on this machine's draw of the operands, before the kernel sees them
    return q, k, v, info, mem, X.expected(q, k, v, info, mem)


@pytest.mark.parametrize("case", X.CASES, ids=[X.case_id(c) for c in X.CASES])
def test_attention_f32_is_exact(dev, case):
    from actionmesh_amd import ops
    q, k, v, info, mem, want = _answer(case.profile, case.shape, case.D, case.scale)
    nseq, H, sq, sk = case.shape
    D, what = case.D, X.case_id(case)
    arenas = {}

    def make(t):
        a = Arena.of(t.to(dev).contiguous(), ld=t.shape[1] + 8)
        arenas[len(arenas)] = (a, a.view.clone())
        return a.view

    q2, k2, v2, kw = X.place(q, k, v, case.layout, make)
    extra = 8 if case.layout == "wide" else 0
    outs = {}
    for kind in KINDS:
        for run in range(2):
            O = Arena(nseq * sq, H * D + extra, torch.float32, dev, ld=H * D + extra + 8)
            got = ops.attention_f32(q2, k2, v2, H, sq, sk, D, scale=case.scale, out=O.view, kind=kind, **kw)
            torch.cuda.synchronize()
            assert got.data_ptr() == O.view.data_ptr()
            O.assert_untouched(f"{what} {kind}: out")               # the gaps behind the rows, the rows behind the last sequence
            if extra:
                pad = O.view[:, H * D:].contiguous().view(torch.int32)
                assert bool((pad == SENTINEL[torch.float32]).all()), f"{what} {kind}: a column past heads * D of the wide out was written"
            outs[kind, run] = O.view[:, :H * D].cpu()
    for a, before in arenas.values():
        a.assert_untouched(f"{what}: an operand's arena")
        assert torch.equal(a.view.view(torch.int32), before.view(torch.int32)), f"{what}: an operand changed"

    first = outs[KINDS[0], 0]
    if case.profile == "ladder":
        assert bool(torch.isfinite(first).all()), f"{what}: output not finite"
        worst = X.ladder_ratio(first, want, -(-sk // X.AK), what)
        assert worst <= 1.0, f"{what}: |out - ref| = {worst:.3f} x the counted bound {X.ladder_bound(-(-sk // X.AK)):.3e} |ref|"
    else:
        rep = X.mismatch_report(first, want, info, mem, what)
        assert rep is None, rep
    for key, o in outs.items():
        assert torch.equal(o.view(torch.int32), first.view(torch.int32)), f"{what}: build / run {key} differs from {(KINDS[0], 0)}"
