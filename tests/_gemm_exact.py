"""GEMM operands on which every fp32 partial sum is exact, the one correct bit pattern of each output, and a CPU emulation of the
epilogues with faults planted at their rounding points.

The argument.  A and W are integers times one power of two (the quantum: 1, or 1/8 for the GELU cases), and for every output element
sum_k |a||w| + |bias| stays below 2^24 quanta.  Every product is then an integer number of quanta, every partial sum of any subset of
them - in any order, any MFMA shape, any K split, started from zero or from the bias - is an integer below 2^24 and therefore exact in
fp32.  gemm_tail_kernel's four K-quarters summed through LDS and the ping-pong kernel's accumulator that starts from the bias change
nothing.  What is left of a kernel is its indexing and its epilogue, and the epilogue has exactly one correct result:

    lin = rnd(exact + bias)                                     rnd: round to nearest even into the 16-bit type
    lin = rnd(exact * rstd_r - mean_r * rstd_r * colsum_n + d_n)        under a folded LayerNorm
    out = lin,  or  rnd(lin + residual)

The fold's ln_stats and ln_colsum are plain inputs of am_gemm_bf16; here mean_r is a small integer, rstd_r a power of two in 2^-3 .. 1,
colsum_n and d_n integers.  Nothing about them is a real LayerNorm; the kernels' fmaf(acc, rstd, fmaf(-mean * rstd, colsum, d)) is exact
on them (every intermediate a multiple of quantum / 8 below 2^24 of those: `conditions`), and that is all that is needed.  A differing
element is a defect of the kernel with certainty; the only thing summation order may change is the sign of a zero, so values are
compared with +0 == -0, and NaN / inf on either side fail.

Operands (`operands`): seeded uniform integers; A and W are independent draws (nothing symmetric: a transposed operand or output
shows).  The ranges (`ranges`) depend on the type and on K so that the integer-valued linear output has a standard deviation of a few hundred (bf16: integers above 256 need rounding) or a few
thousand (f16: above 2048) at every K - a fifth or more of the outputs are not representable, a twentieth or more are exact ties, and
ties fall on both sides (`conditions` asserts the shares on the operands alone, before any kernel sees them).  Row r % 37 == 5 of A and
row n % 29 == 3 of W are zero and the bias holds +0.0 in columns n % 29 in (3, 11): exact zeros in the output.  The bias, the
fold's shift and the residual are small against the outputs that need rounding (|bias| <= 32 against 256 in bf16), so that a
misplaced rounding stays inside the tolerance the other GEMM tests use - tests/test_gemm_exact_cpu.py shows that it does, and that the
exact comparison rejects it.

GELU.  The pre-activation lin is known to the bit, the activation's evaluation is not.  The quantum is 1/8 and the ranges are narrow:
lin is a multiple of 1/8 (of 1/64 under a fold, before its rounding) within about +-12, which covers the table range of the 256x256
tile, |x| >= 8 and exact zeros (both take the arithmetic branch).  Expected g = gelu_fp64(lin); per-element bound
u |g| + (1 + u) E with u the unit roundoff of the output (2^-8 / 2^-11) and E = GELU_E, the absolute error
actionmesh_amd/csrc/am_common.h states for gelu_erf - taken from that comment, not fitted.  GELU cases are exempt from the rounding
shares, as are shapes of fewer than 4096 outputs.  NOT pinned by these cases: the rounding of the linear IN FRONT of the activation.
In every GELU case, fold + GELU included, the value the linear rounds is representable in both types (the rows with rstd = 1/8, whose
values are odd multiples of 1/64, stay below 4, where bf16 still holds them), so a kernel that applied GELU to the unrounded
pre-activation would pass; an unrepresentable pre-activation would move g by up to half a spacing of its input, the size of the
bound's own u |g|, and the comparison could not tell the two apart.  That rounding point is pinned by the cases without GELU.

Largest |out - g| / bound seen on the MI355X (first run of tests/test_gemm_exact_gpu.py, every GELU case inside the bound): bf16 0.967
(fold + GELU on the ping-pong tile and the rows behind it, lin = 2.078125: g lies next to a tie of the output's rounding, so the ratio
is the rounding's share u |g|, not gelu_erf's error), f16 0.920 (ping-pong fold + GELU, lin = -2.484375); GELU without a fold: bf16
0.840 at lin = 0.75 in every kernel.  GELU_WORST below."""
import collections
import functools
import math

import torch

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
SIG_BITS = {"bf16": 8, "f16": 11}                   # significand bits, the implicit one included
U_OUT = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}      # unit roundoff
GELU_E = 3.3e-7                                     # am_common.h, gelu_erf: "|error| <= 3.3e-7 absolute"
GELU_WORST = {"bf16": 0.967, "f16": 0.920}          # max |out - g| / bound of the first GPU run (a record, not a threshold)
SENTINEL = 7.0                                      # rows a c_map skips
ZERO_ROW_A, ZERO_ROW_W, ZERO_BIAS = (37, 5), (29, 3), (29, (3, 11))

EPILOGUES = ("plain", "bias", "bias_res", "res_inplace", "fold", "fold_d", "fold_d_res", "gelu", "fold_gelu")

# kernel: k128 (force_small), lockstep (force_big + legacy), pingpong (force_big), dispatch (no switch), tail (force_big, M = 2048 + r:
# rows 2048.. go to gemm_tail_kernel), tail128 (the same with a c_map: the remainder rows fall back to the 128x128 kernel).
# k1: split-A boundary (0: one A).  a_map / c_map: (G, group_stride, offset).  skew: the start-skew field of `act` (0: the library's).
Case = collections.namedtuple("Case", "kernel M N K epi k1 a_map c_map skew", defaults=(0, None, None, 0))
TILE = {"k128": (128, 128), "lockstep": (256, 256), "pingpong": (256, 256), "dispatch": (256, 256), "tail": (32, 64), "tail128": (128, 128)}


def _cases():
    c = []
    # 128x128: M and N tails with N % 128 != 0 on every shape; 1, 3 and 16 k-tiles
    s1, s2, s3 = (37, 64, 64), (129, 136, 192), (300, 328, 1024)
    for shape, epis in ((s1, ("plain", "fold", "gelu")), (s2, ("bias", "res_inplace", "fold_d", "fold_gelu")),
                        (s3, ("bias_res", "fold_d_res", "gelu"))):
        c += [Case("k128", *shape, e) for e in epis]
    c += [Case("k128", 129, 136, 192, "bias", k1=64),
          Case("k128", 144, 136, 64, "fold_d", a_map=(48, 49, 1)),          # the statistics follow the mapped A row
          Case("k128", 144, 136, 64, "res_inplace", c_map=(48, 49, 1))]
    # 256x256 lockstep (no fold: the entry refuses it): one full tile; M and N tails; 1, 3, 16 k-tiles
    l1, l2, l3 = (256, 256, 64), (777, 328, 192), (1300, 520, 1024)
    for shape, epis in ((l1, ("plain", "bias_res")), (l2, ("plain", "bias", "bias_res", "res_inplace", "gelu")), (l3, ("bias", "gelu"))):
        c += [Case("lockstep", *shape, e) for e in epis]
    # 256x256 ping-pong: 1 .. 64 k-tiles (prologue only, steady state, clamped last stages), the full-tile fast store and the edge path
    for shape, epis in ((l1, ("plain", "bias_res", "gelu")), (l2, EPILOGUES), (l3, ("bias", "fold_d", "res_inplace", "fold_gelu")),
                        ((256, 256, 4096), ("plain", "bias_res")), ((2304, 256, 128), ("fold_d_res", "gelu"))):
        c += [Case("pingpong", *shape, e) for e in epis]
    c += [Case("pingpong", 777, 328, 192, "bias", k1=64),
          Case("pingpong", 1440, 328, 192, "bias", a_map=(48, 49, 1)),
          Case("pingpong", 1440, 328, 192, "res_inplace", c_map=(48, 49, 1))]
    # its own dispatch: 17 x 12 = 204 tiles and one remainder row.  At 204 tiles the library's own start skew is 0 units (it begins at
    # 4 rounds of 256 tiles), so the second case sets the field to the 4 units the model's largest linears get.
    c += [Case("dispatch", 4097, 3072, 64, "bias_res"), Case("dispatch", 4097, 3072, 64, "fold_d", skew=4)]
    # gemm_tail_kernel: r = 33 / 128 fill 2 / 4 row blocks with a partial one; N = 328 leaves a 64-column block of 8 columns; K = 64
    # makes a K-quarter of one 16-step, K = 576 a quarter of 144 = one group of eight steps and a short one.
    # The first ten are a diagonal over r x N x K; the rest see to it that EVERY epilogue meets a partial row block (r = 1 or 33, next
    # to the kernel's early return) and the 8-column last block (N = 328, where the 4-wide bias / colsum / residual loads and the 8-byte
    # store sit against the edge) - tests/test_gemm_exact_cpu.py holds the table to that.
    for r, N, K, e in ((1, 64, 64, "plain"), (32, 328, 576, "bias"), (33, 328, 1024, "bias_res"), (128, 64, 576, "res_inplace"),
                       (33, 64, 64, "fold"), (128, 328, 1024, "fold_d"), (1, 328, 576, "fold_d_res"), (32, 64, 1024, "gelu"),
                       (33, 328, 576, "fold_gelu"), (128, 328, 64, "bias_res"),
                       (33, 328, 64, "plain"), (1, 328, 1024, "bias"), (33, 328, 1024, "res_inplace"), (1, 328, 64, "fold"),
                       (33, 328, 576, "fold_d"), (33, 328, 576, "gelu")):
        c.append(Case("tail", 2048 + r, N, K, e))
    c.append(Case("tail", 2048 + 33, 328, 576, "bias", k1=192))             # the A1 / A2 boundary inside K-quarter 1 (144 .. 288)
    c.append(Case("tail128", 2048 + 32, 328, 64, "bias_res", c_map=(32, 33, 1)))
    return c


CASES = _cases()
Built = collections.namedtuple("Built", "case name q gelu fold w exact absum aidx cidx rows_c a2 bias res stats colsum a")


def case_id(c):
    s = f"{c.kernel}-{c.M}x{c.N}x{c.K}-{c.epi}"
    return s + (f"-k1_{c.k1}" if c.k1 else "") + ("-amap" if c.a_map else "") + ("-cmap" if c.c_map else "") + (f"-skew{c.skew}" if c.skew else "")


def ranges(name, K, gelu):
    """(ra, rw): A holds integers in [-ra, ra], W in [-rw, rw] (times the quantum)."""
    if gelu:
        assert K <= 1024, "no GELU operands for K > 1024"
        return (2, 4) if K <= 64 else (1, 5) if K <= 128 else (1, 4) if K <= 256 else (1, 2) if K <= 640 else (1, 1)
    if name == "bf16":      # standard deviation of the output: 725 .. 1451 | 576 at K = 576 | 405 at 1024, 810 at 4096
        return (16, 16) if K <= 256 else (8, 8) if K <= 640 else (4, 8)
    return (32, 32) if K <= 256 else (24, 24) if K <= 640 else (16, 16)      # f16: 2816 .. 5632 | 4800 | 2900, 5800


def rnd(x, name):
    """Round to nearest even into the 16-bit type (torch's conversion), back in fp64."""
    return x.to(DTYPES[name]).double()


def map_rows(M, m):
    """Physical row of every logical row under the row map (G, group_stride, offset); None: the identity."""
    r = torch.arange(M)
    return r if not m else (r // m[0]) * m[1] + m[2] + r % m[0]


def phys_rows(M, m):
    return M if not m else (M // m[0]) * m[1]


def _ints(g, shape, r):
    return torch.randint(-r, r + 1, shape, generator=g).double()


@functools.lru_cache(maxsize=3)
def _a_w(name, M, N, K, gelu, a_map):
    """(A (physical rows, K), W (N, K), exact = A[logical rows] W^T (M, N)) in fp64, shared by the epilogues of a shape."""
    ra, rw = ranges(name, K, gelu)
    q = 0.125 if gelu else 1.0
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
    rows_a = phys_rows(M, a_map)
    a = _ints(g, (rows_a, K), ra)
    w = _ints(g, (N, K), rw) * q
    a[torch.arange(rows_a) % ZERO_ROW_A[0] == ZERO_ROW_A[1]] = 0.0
    w[torch.arange(N) % ZERO_ROW_W[0] == ZERO_ROW_W[1]] = 0.0
    aidx = map_rows(M, a_map)
    al = a[aidx]
    exact = al @ w.T                                      # fp64 on integers below 2^53 quanta: exact
    absum = al.abs() @ w.abs().T
    return a, w, exact, absum


def operands(case, name, small_shift=False):
    """Everything of `case` in the type `name`, on the CPU in fp64 (each value exact in its storage format): a, a2, w, bias (or the
    fold's d), res, stats, colsum, the row indices, `exact`, and the expected `lin` / `want` of `reference`.
    small_shift (tests/test_gemm_exact_cpu.py only): |bias|, |mean colsum| <= 1 (8 in f16), one spacing of the smallest outputs that
    round - a shift that cannot pull an output across a power of two by more than the other tests' atol forgives."""
    epi = case.epi
    gelu, fold = epi.endswith("gelu"), epi.startswith("fold")
    q = 0.125 if gelu else 1.0
    big = 1 if name == "bf16" or gelu else 8              # f16 rounds above 2048 where bf16 rounds above 256
    M, N, K = case.M, case.N, case.K
    a, w, exact, absum = _a_w(name, M, N, K, gelu, case.a_map)
    g = torch.Generator().manual_seed(7919 * M + 31 * N + K + 17 * EPILOGUES.index(epi))
    c = dict(case=case, name=name, q=q, gelu=gelu, fold=fold, w=w, exact=exact, absum=absum, aidx=map_rows(M, case.a_map),
             cidx=map_rows(M, case.c_map), rows_c=phys_rows(M, case.c_map), a2=None, bias=None, res=None, stats=None, colsum=None)
    c["a"], c["a2"] = (a[:, :case.k1].contiguous(), a[:, case.k1:].contiguous()) if case.k1 else (a, None)
    cols = torch.arange(N)
    zero_b = (cols % ZERO_BIAS[0] == ZERO_BIAS[1][0]) | (cols % ZERO_BIAS[0] == ZERO_BIAS[1][1])
    if fold:
        rows_a = a.shape[0]
        mean = _ints(g, (rows_a,), 1 if gelu or small_shift else 2)
        mean[torch.arange(rows_a) % ZERO_ROW_A[0] == ZERO_ROW_A[1]] = 0.0
        rstd = torch.exp2(-torch.randint(0, 4, (rows_a,), generator=g).double())
        c["stats"] = torch.stack([mean, rstd], 1)
        c["colsum"] = _ints(g, (N,), big if small_shift else 8 * big) * q
        c["colsum"][cols % ZERO_ROW_W[0] == ZERO_ROW_W[1]] = 0.0
        if epi != "fold":
            assert not small_shift
            c["bias"] = _ints(g, (N,), 8 if gelu else 5 * big) * q
    elif epi not in ("plain", "res_inplace"):
        c["bias"] = _ints(g, (N,), 16 if gelu else big if small_shift else 32 * big) * q
    if c["bias"] is not None:
        c["bias"][zero_b] = 0.0
    if "res" in epi:                                      # integer-valued and exact in the type
        c["res"] = rnd(_ints(g, (c["rows_c"], N), 500 * big), name)
    c = Built(**c)
    lin, want = reference(c)
    return c, lin, want


def pre_rounding(c):
    """The value the linear rounds, in fp64 (exact), and under a fold the FMA intermediates."""
    if c.fold:
        st = c.stats[c.aidx]
        mean, rstd = st[:, :1], st[:, 1:]
        nm = -mean * rstd
        inner = nm * c.colsum + (c.bias if c.bias is not None else 0.0)
        return c.exact * rstd + inner, (nm, inner)
    return c.exact + (c.bias if c.bias is not None else 0.0), None


def gelu_fp64(x):
    return x * 0.5 * torch.special.erfc(-x * math.sqrt(0.5))


def reference(c):
    """(lin, want) in fp64 on the CPU: lin = rnd(exact + bias) or the fold's form; want = lin, gelu_fp64(lin) (GELU: compare with
    `gelu_check`) or rnd(lin + res).  (M, N) logical rows: the caller scatters with c.cidx."""
    v, _ = pre_rounding(c)
    lin = rnd(v, c.name)
    if c.gelu:
        return lin, gelu_fp64(lin)
    if c.res is not None:
        return lin, rnd(lin + c.res[c.cidx], c.name)
    return lin, lin


def rounding_facts(v, name):
    """Shares of the values v (fp64) that are not representable in the type, that are exact ties, and ties rounded up / down in
    magnitude.  Normal range only (asserted)."""
    p = SIG_BITS[name]
    r = rnd(v, name)
    nz = v != 0
    assert name == "bf16" or float(v[nz].abs().min() if bool(nz.any()) else 1.0) >= 2.0 ** -14, "a subnormal f16 value"
    _, e = torch.frexp(v)                                 # |v| = m 2^e, m in [0.5, 1): the spacing of v's binade is 2^(e - p)
    units = v.abs() * torch.exp2((p - e).double())        # |v| in spacings: in [2^(p-1), 2^p)
    tie = nz & (units - units.floor() == 0.5)
    n = v.numel()
    return dict(needs_rounding=float((r != v).sum()) / n, ties=float(tie.sum()) / n, ties_up=float((tie & (r.abs() > v.abs())).sum()) / n,
                ties_down=float((tie & (r.abs() < v.abs())).sum()) / n, zeros=int((r == 0).sum()), std=float(v.std()) if n > 1 else 0.0)


def _is_int(x, q=1.0):
    return bool((x / q == (x / q).round()).all())


def conditions(c):
    """What the operands promise (module docstring), asserted in fp64 on the operands alone.  Returns the measured facts."""
    name, q = c.name, c.q
    dt = DTYPES[name]
    # 1. every operand is exact in its storage format
    for what, t in (("a", c.a), ("a2", c.a2), ("w", c.w), ("res", c.res)):
        assert t is None or torch.equal(t.to(dt).double(), t), f"{what} is not exact in {name}"
    for what, t in (("bias", c.bias), ("stats", c.stats), ("colsum", c.colsum)):
        assert t is None or torch.equal(t.float().double(), t), f"{what} is not exact in fp32"
    assert _is_int(c.a) and (c.a2 is None or _is_int(c.a2)) and _is_int(c.w, q) and (c.bias is None or _is_int(c.bias, q))
    assert c.res is None or _is_int(c.res, q)
    # 2. every partial sum, in any order and started from the bias or not, is an integer below 2^24 quanta
    top = c.absum + (c.bias.abs() if c.bias is not None else 0.0)
    assert float(top.max()) < 2.0 ** 24 * q, f"sum |a||w| + |bias| reaches {float(top.max()) / q} quanta"
    v, fma = pre_rounding(c)
    if c.fold:
        qf = q / 8                                        # rstd >= 2^-3
        rstd = c.stats[:, 1]
        assert bool(((rstd == 1) | (rstd == 0.5) | (rstd == 0.25) | (rstd == 0.125)).all()) and _is_int(c.stats[:, 0]) and _is_int(c.colsum, q)
        assert _is_int(fma[0], 0.125)                     # -mean rstd: one rounding-free product
        for what, t in (("fma(-mean rstd, colsum, d)", fma[1]), ("fma(acc, rstd, .)", v), ("acc rstd", c.exact * c.stats[c.aidx][:, 1:])):
            assert _is_int(t, qf) and float(t.abs().max()) < 2.0 ** 24 * qf, f"{what} is not exact in fp32"
    lin, want = reference(c)
    # 3. finite, and inside the type's range
    limit = 65504.0 if name == "f16" else 3.0e38
    for t in (lin, want) + ((lin + c.res[c.cidx],) if c.res is not None else ()):
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) <= limit
    facts = rounding_facts(v, name)
    facts["outputs"] = v.numel()
    n = v.numel()
    if c.gelu:          # exempt from the shares: lin is (nearly always) exact.  What matters is the range it covers
        facts.update(max_abs=float(lin.abs().max()), beyond_table=int((lin.abs() >= 8).sum()), in_table=int(((lin.abs() < 8) & (lin != 0)).sum()))
        assert _is_int(lin, q / 8) and facts["max_abs"] <= 24.0 and facts["in_table"] > n // 2
        assert n < 4096 or facts["beyond_table"] > 0, "no pre-activation outside the GELU table's range"
    elif n >= 4096:     # 4. the rounding is exercised (smaller shapes are exempt)
        assert facts["needs_rounding"] >= 0.20 and facts["ties"] >= 0.05 and facts["ties_up"] >= 0.02 and facts["ties_down"] >= 0.02, facts
    # 5. exact zeros
    assert facts["zeros"] > 0, "no output is exactly zero"
    return facts


# ---- comparison ---------------------------------------------------------------------------------------------------------------------
def mismatch_report(out, want, tile, exact=None, what="", name=None):
    """The text of the assertion (None when out equals want: values, +0 == -0, nothing non-finite): how many elements differ, the
    first few as (row, col, got, want, exact value), the residues of row mod tile and col mod tile that hold them, and whether every
    mismatch is a tie - a lane, a tile edge or a rounding mode."""
    out, want = out.double().cpu(), want.double().cpu()
    bad = (out != want) | ~torch.isfinite(out) | ~torch.isfinite(want)
    if not bool(bad.any()):
        return None
    rows, cols = bad.nonzero(as_tuple=True)
    tm, tn = tile
    lines = [f"{what}: {int(bad.sum())} of {bad.numel()} elements differ ({int((~torch.isfinite(out)).sum())} not finite)"]
    for r, cidx in list(zip(rows.tolist(), cols.tolist()))[:8]:
        ex = f", exact {float(exact[r, cidx])!r}" if exact is not None else ""
        lines.append(f"  ({r}, {cidx}): got {float(out[r, cidx])!r}, want {float(want[r, cidx])!r}{ex}")
    rm, cm = sorted(set((rows % tm).tolist())), sorted(set((cols % tn).tolist()))
    lines.append(f"  row % {tm}: {rm if len(rm) <= 32 else f'{len(rm)} residues, {rm[0]} .. {rm[-1]}'}; "
                 f"col % {tn}: {cm if len(cm) <= 32 else f'{len(cm)} residues, {cm[0]} .. {cm[-1]}'}; "
                 f"rows {int(rows.min())} .. {int(rows.max())}, cols {int(cols.min())} .. {int(cols.max())}")
    if exact is not None and name is not None:
        v = exact[rows, cols].double()
        _, e = torch.frexp(v)
        units = v.abs() * torch.exp2((SIG_BITS[name] - e).double())
        lines.append(f"  every mismatch a tie of the {name} rounding: {bool(((units - units.floor()) == 0.5).all())}")
    return "\n".join(lines)


def gelu_check(out, lin, name, what=""):
    """(max |out - gelu_fp64(lin)| / bound, assertion text or None); bound = u |g| + (1 + u) E per element."""
    out, g = out.double().cpu(), gelu_fp64(lin)
    u = U_OUT[name]
    bound = u * g.abs() + (1.0 + u) * GELU_E
    ratio = (out - g).abs() / bound
    ratio = torch.where(torch.isfinite(out), ratio, torch.full_like(ratio, float("inf")))
    at = int(ratio.argmax())
    r, cidx = divmod(at, out.shape[1])
    worst = float(ratio.flatten()[at])
    print(f"exact-gemm GELU {what}: max err / bound {worst:.3f} at ({r}, {cidx}), lin {float(lin[r, cidx])!r}")
    if worst <= 1.0:
        return worst, None
    return worst, (f"{what}: {int((ratio > 1).sum())} elements outside u |g| + (1 + u) E; worst {worst:.3f} x bound at ({r}, {cidx}): "
                   f"lin {float(lin[r, cidx])!r}, got {float(out[r, cidx])!r}, gelu {float(g[r, cidx])!r}")


# ---- CPU emulation of the epilogue, in fp32 torch with the kernels' rounding points ---------------------------------------------------
# truncate / half_away: the linear's rounding goes toward zero / rounds ties away from zero (the residual add keeps nearest even)
FAULTS = ("truncate", "half_away", "bias_after_rounding", "residual_before_rounding", "fold_rounded_twice", "one_k_step_dropped")
ORDERS = ("ascending", "quarters", "from_bias")


def _round_with(x, name, mode):
    """fp32 -> the 16-bit type -> fp32: nearest even (torch), toward zero, or half away from zero.  Normal range."""
    if mode == "nearest_even":
        return x.to(DTYPES[name]).float()
    v = x.double()
    _, e = torch.frexp(v)
    sp = torch.exp2((e - SIG_BITS[name]).double())
    u = v.abs() / sp
    u = u.floor() if mode == "truncate" else (u + 0.5).floor()
    return (v.sign() * u * sp).float()


def emulate(c, order="ascending", fault=None):
    """The linear and its epilogue as the kernels compute them: fp32 accumulation over 16-wide k-steps in `order` (ascending from zero;
    four K-quarters, each descending, summed (q0 + q1) + (q2 + q3); ascending from the bias - only without a fold, as in the ping-pong
    kernel), then the rounding points of am_gemm.hip.  -> fp32 (M, N) logical rows.  `fault`: one of FAULTS."""
    assert order in ORDERS and fault in (None,) + FAULTS and not c.gelu
    name = c.name
    a = (torch.cat([c.a, c.a2], 1) if c.a2 is not None else c.a)[c.aidx].float()
    w = c.w.float()
    K = a.shape[1]
    steps = list(range(0, K, 16))
    bias = c.bias.float() if c.bias is not None else None

    def partial(k0, rows=slice(None)):
        return a[rows, k0:k0 + 16] @ w[:, k0:k0 + 16].T

    def chain(ks, start):
        acc = start
        for k0 in ks:
            p = partial(k0)
            if fault == "one_k_step_dropped" and k0 == steps[len(steps) // 2]:
                p[32:64] = 0.0                            # one 32-row block loses one k-step
            acc = acc + p
        return acc

    zero = torch.zeros((a.shape[0], w.shape[0]))
    bias_in_acc = order == "from_bias" and bias is not None and not c.fold and fault != "bias_after_rounding"
    if order == "quarters":
        kq = K // 4
        qs = [chain([k for k in reversed(steps) if i * kq <= k < (i + 1) * kq], zero) for i in range(4)]
        acc = (qs[0] + qs[1]) + (qs[2] + qs[3])
    else:
        acc = chain(steps, zero + bias if bias_in_acc else zero)
    mode = fault if fault in ("truncate", "half_away") else "nearest_even"
    res = c.res[c.cidx].float() if c.res is not None else None
    if c.fold:
        st = c.stats[c.aidx].float()
        mean, rstd = st[:, :1], st[:, 1:]
        inner = (-mean * rstd) * c.colsum.float() + (bias if bias is not None else 0.0)      # exact: an fma would give the same
        if fault == "fold_rounded_twice":
            lin = _round_with(_round_with(acc * rstd, name, mode) + inner, name, mode)
        else:
            lin = _round_with(acc * rstd + inner, name, mode)
    else:
        assert fault != "fold_rounded_twice"
        if fault == "bias_after_rounding":
            lin = _round_with(_round_with(acc, name, mode) + bias, name, mode)
        elif fault == "residual_before_rounding":
            return _round_with(acc + (0.0 if bias is None or bias_in_acc else bias) + res, name, mode)
        else:
            lin = _round_with(acc if bias is None or bias_in_acc else acc + bias, name, mode)
    if res is None:
        return lin
    assert fault != "residual_before_rounding" or not c.fold
    return _round_with(lin + res, name, "nearest_even")          # truncate / half_away are faults of the linear's rounding
