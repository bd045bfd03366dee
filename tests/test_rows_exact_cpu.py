"""The exact-rows yardstick of tests/test_rows_exact_gpu.py, tested without a GPU: the operands keep their promises at every shape
and type the GPU file uses, the CPU emulation of the row kernels stays inside the per-element bound, and planted faults are rejected
by that bound.  For every fault the criterion of the existing test of the same kernel is applied to that test's own operands, and
the verdict printed: the first six are the gap the existing suite leaves (asserted accepted where they are)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _rows_exact as X

STORES = ["bf16", "f16"]
HEAD_SHAPES = [(2, 2, 49, 1), (1, 1, 130, 3)]
# (kernel, storage of the rows, output type, widths, ladder)
KERNELS = [("layernorm", "bf16", "bf16", X.WIDTHS, X.LADDER), ("layernorm", "f16", "f16", X.WIDTHS, X.LADDER),
           ("add_layernorm_f32", "f32", "bf16", X.WIDTHS, X.LADDER), ("add_layernorm_f32", "f32", "f16", X.WIDTHS, X.LADDER),
           ("layernorm_f32", "f32", "f32", X.WIDTHS_F32, X.LADDER_F32)]
KERNEL_IDS = [f"{k[0]}-{k[1]}-{k[2]}" for k in KERNELS]


def test_offsets_are_the_largest_the_formats_allow():
    assert (X.offset_of("bf16"), X.offset_of("f16"), X.offset_of("f32")) == (509.0, 2047.0, 2047.0)
    assert X.eps32(0.25) == 0.25 and X.eps32(1e-5) != 1e-5


def test_switch_widths_are_the_launch_ladders():
    """Both sides of every switch of NCH: ceil(C / 512) in {1, 2, 4, 8} (8 columns per lane), ceil(C / 256) in {1 .. 16} (4 per lane)."""
    for ladder, step, widths, top in ((X.LADDER, 8, X.WIDTHS, 8), (X.LADDER_F32, 4, X.WIDTHS_F32, 16)):
        n = 1
        while n < top:
            assert ladder * n in widths and ladder * n + step in widths, (ladder, n)
            n *= 2
        assert 4096 in widths and step in widths


@pytest.mark.parametrize("mode", ["cycle", "unit"])
@pytest.mark.parametrize("fmt", ["bf16", "f16", "f32"])
def test_rows_keep_their_conditions(fmt, mode):
    for rows in X.ROWS:
        for C in sorted(set(X.WIDTHS + (X.WIDTHS_F32 if fmt == "f32" else []))):
            op = X.rows_operands(rows, C, fmt, mode, seed=rows + C)       # asserts rows_conditions itself
            facts = X.rows_conditions(op)
            if mode == "cycle":
                assert [X.CYCLE[i] for i in op["profile"][:4].tolist()] == list(X.CYCLE)
                off = op["m"][op["profile"] == 1]
                assert bool((off.abs() == X.offset_of(fmt)).all()) and (rows < 8 or float(off.min()) < 0 < float(off.max()))
                var = (op["x"] - op["m"][:, None]).pow(2).mean(-1)
                assert float(var[op["profile"] == 2].max()) < X.eps32(X.EPS) and bool((var[op["profile"] == 3] == 0).all())
            else:
                assert bool(((op["x"] - op["m"][:, None]).pow(2).mean(-1) + X.eps32(op["eps"]) == 1.0).all())
        print(f"{fmt} {mode} {rows} x {C}: {facts}")


def test_weights_are_dyadic_and_nocancel_does_not_cancel():
    for mode in X.B_MODES:
        w, b = X.weights(4096, mode, seed=5)
        assert torch.equal(w * 8, (w * 8).round()) and torch.equal(b * 8, (b * 8).round())
        assert float(w.abs().min()) == 0.5 and float(w.abs().max()) == 1.875
        for call in ("cycle", "unit"):
            op = X.rows_operands(131, 4096, "bf16", call, seed=9)
            X.ln_reference(op["x"], w, b, op["eps"])                            # asserts the quarter for "nocancel"
    assert float(X.weights(64, "zero", 1)[1].abs().max()) == 0 and float(X.weights(64, "nocancel", 1)[1].abs().min()) >= 5


def test_spacing_is_the_formats():
    v = torch.tensor([0.0, 1.0, 1.5, 2.0, -3.0, 2.0 ** -14, 2.0 ** -20, 1000.0], dtype=torch.float64)
    assert X.spacing(v, "bf16").tolist() == [2.0 ** -133, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -21, 2.0 ** -27, 4.0]
    assert X.spacing(v, "f16").tolist() == [2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -9, 2.0 ** -24, 2.0 ** -24, 0.5]
    for fmt, (dt, _, _) in X.FORMATS.items():
        x = torch.tensor([1.0, 1.75, 640.0, 0.01], dtype=dt)
        up = torch.nextafter(x.float(), torch.tensor(float("inf"))) if dt == torch.float32 else None
        if up is not None:
            assert torch.equal((up - x).double(), X.spacing(x.double(), fmt))


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
def test_emulated_layernorms_stay_inside_the_bound(kernel):
    name, store, out_fmt, widths, _ = kernel
    worst = 0.0
    for rows in X.ROWS:
        for C in widths:
            for call in ("cycle", "unit"):
                op = X.rows_operands(rows, C, store, call, seed=rows + C)
                for b_mode in X.B_MODES:
                    w, b = X.weights(C, b_mode, seed=C)
                    ref, term = X.ln_reference(op["x"], w, b, op["eps"])
                    out = X.emulate_layernorm(op["x"], w, b, op["eps"], out_fmt)
                    worst = max(worst, X.check(out, ref, X.ln_bound(ref, term, out_fmt), f"emulated {name} {out_fmt} {rows}x{C} {call} {b_mode}"))
                    const = op["profile"] == 3
                    assert torch.equal(out[const].double(), X.rnd(b.double(), out_fmt).expand(int(const.sum()), C)), "a constant row gives b"
    print(f"emulated {name} {store} -> {out_fmt}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("store", STORES)
def test_emulated_statistics_stay_inside_the_bound(store):
    from oracle import row_stats_oracle as RO
    for C in X.WIDTHS:
        for call in ("cycle", "unit"):
            op = X.rows_operands(131, C, store, call, seed=C)
            st = X.emulate_row_stats(op["x"], op["eps"])
            X.stats_check(st, op["x"], op["eps"], False, f"emulated two-pass statistics {store} {C} {call}")
            if C % 256 == 8:                                                     # a short last slice of 8 columns, merged like the others
                st32 = torch.stack(X.stats_reference(op["x"], op["eps"]), -1).float()
                X.stats_check(st32, op["x"], op["eps"], True, f"merged statistics, rounded fp64 {store} {C} {call}")
            if C % 256 == 0:
                parts, _ = X.slice_parts(op["x"])                                # asserts the parts exact in fp32
                mean, rstd, oparts = RO.row_stats(op["x"].float().numpy(), eps=op["eps"])
                assert np.array_equal(oparts.astype(np.float64), parts.numpy()), "the canonical slices of these rows are exact"
                st = torch.from_numpy(np.stack((mean, rstd), -1))
                X.stats_check(st, op["x"], op["eps"], True, f"canonical statistics (numpy restatement) {store} {C} {call}")
    op = X.rows_operands(131, 4096, store, "unit", seed=1)
    assert bool((X.emulate_row_stats(op["x"], op["eps"])[:, 1] == 1.0).all()), "unit rows: var + eps = 1"


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_emulated_head_split_stays_inside_the_bound(shape, store):
    nseq, fps, L, heads = shape
    seq_len, rows = fps * L, nseq * fps * L
    x, prof = X.head_operands(rows, heads, 3, store, seed=L)
    wq, wk = X.head_weights(seed=L + 1)
    tables = X.rope_tables(nseq * fps, seed=L + 2)
    for norm in (True, False):
        for rope in (tables, None):
            for part, w in ((0, wq), (1, wk)):
                w = w if norm else None
                ref, terms = X.head_reference(x, heads, 3, part, w, rope, seq_len, L)
                out = X.emulate_head(x, heads, 3, part, w, rope, seq_len, L, store)
                X.head_check(out, ref, terms, store, norm, rope is not None, prof, f"emulated head split {store} {shape} part {part} norm={norm} rope={rope is not None}")


@pytest.mark.parametrize("store", STORES)
def test_emulated_fold_is_exact(store):
    for N in (1, 5):
        for K in (8, 64, 72, 320):
            W, gamma, beta, bias = X.fold_operands(N, K, seed=N + K)
            for bs in (bias, None):
                wf, cs, d = X.emulate_fold(W, gamma, beta, bs, store)
                rwf, rcs, rd = X.fold_reference(W, gamma, beta, bs)
                assert torch.equal(wf.double(), rwf) and torch.equal(cs.double(), rcs) and torch.equal(d.double(), rd)


# ---- planted faults ---------------------------------------------------------------------------------------------------------------
def _old_layernorm(fault, out_fmt):
    """tests/test_kernels_gpu.py::test_layernorm / test_f16_kernels_gpu.py::test_layernorm_f16 on their own operands (64 rows of
    each width): 1.5 u |ref| + 1e-5 per element against fp32 layer_norm.  -> {C: accepted}."""
    u = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}[out_fmt]
    verdict = {}
    for C in (256, 1024, 2048, 4096):
        g = torch.Generator().manual_seed(C)
        x = (torch.randn((64, C), generator=g) * 2.0 + 0.5).to(X.FORMATS[out_fmt][0])
        w, b = torch.randn((C,), generator=g) * 0.2 + 1.0, torch.randn((C,), generator=g) * 0.2
        ref = F.layer_norm(x.float(), (C,), w, b, 1e-5)
        out = X.emulate_layernorm(x, w, b, 1e-5, out_fmt, fault=fault).float()
        verdict[C] = not bool(((out - ref).abs() > 1.5 * u * ref.abs() + 1e-5).any())
    return verdict


def _old_add_layernorm(fault, out_fmt):
    """tests/test_kernels_gpu.py::test_add_layernorm_f32 on its own operands (64 rows): max-abs 2^-7 / 2^-10 of max|z| and rel-L2."""
    verdict = {}
    for C in (1024, 320, 2048):
        g = torch.Generator().manual_seed(C)
        h = torch.randn((64, C), generator=g) * 3 + 2 + torch.randn((64, C), generator=g).to(X.FORMATS[out_fmt][0]).float()
        w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
        ref = F.layer_norm(h, (C,), w, b, 1e-5)
        out = X.emulate_layernorm(h, w, b, 1e-5, out_fmt, fault=fault).float()
        mx = float((out - ref).abs().max()) <= 2.0 ** (-7 if out_fmt == "bf16" else -10) * float(ref.abs().max())
        verdict[C] = mx and float((out - ref).norm() / ref.norm()) < (2.5e-3 if out_fmt == "bf16" else 3.5e-4)
    return verdict


def _old_layernorm_f32(fault):
    """tests/test_fp32_path_gpu.py::test_layernorm_f32_against_fp64: 4 fp32 ulp of |w| (|x| + |mean|) rstd + |b| against fp64."""
    verdict = {}
    for C in (1024, 4096, 100):
        g = torch.Generator().manual_seed(C)
        x = torch.randn((64, C), generator=g) * 3 + 0.5
        w, b = torch.randn((C,), generator=g), torch.randn((C,), generator=g)
        xd = x.double()
        mean = xd.mean(-1, keepdim=True)
        rstd = (xd.var(-1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
        ref = (xd - mean) * rstd * w.double() + b.double()
        tol = 4 * 2.0 ** -23 * (w.double().abs() * (xd.abs() + mean.abs()) * rstd + b.double().abs())
        verdict[C] = not bool(((X.emulate_layernorm(x, w, b, 1e-5, "f32", fault=fault, ladder=X.LADDER_F32).double() - ref).abs() > tol).any())
    return verdict


# The faults the existing criteria must accept.  C - 1 for C is not among them: where w xhat and b cancel, its 1 / (2 C) of |w xhat|
# stands above the 1e-5 absolute term of test_layernorm (rejected at every width of that test, both types), and above the rel-L2 clause
# of test_add_layernorm_f32 at C = 320 and 1024 in f16
GAP = [f for f in X.LN_FAULTS[:6] if f != "c_minus_1"]


# fp32 -> f16 -> bf16 is a fault of the bf16 output alone
LN_FAULT_CASES = [pytest.param(f, k, id=f"{f}-{i}") for f in X.LN_FAULTS for k, i in zip(KERNELS, KERNEL_IDS) if f != "rounded_twice" or k[2] == "bf16"]


@pytest.mark.parametrize("fault,kernel", LN_FAULT_CASES)
def test_planted_layernorm_faults_fail_the_bound(fault, kernel):
    name, store, out_fmt, widths, ladder = kernel
    C = ladder + (8 if ladder == X.LADDER else 4) if fault == "ladder_off_by_one" else 4096
    op = X.rows_operands(131, C, store, "cycle", seed=3)
    w, b = X.weights(C, "general", seed=4)
    ref, term = X.ln_reference(op["x"], w, b, op["eps"])
    bnd = X.ln_bound(ref, term, out_fmt)
    good = X.emulate_layernorm(op["x"], w, b, op["eps"], out_fmt, ladder=ladder)
    assert X.ratio(good, ref, bnd, f"{name} {store}->{out_fmt} fault-free")[0] <= 1.0
    bad = X.emulate_layernorm(op["x"], w, b, op["eps"], out_fmt, fault=fault, ladder=ladder)
    worst, place = X.ratio(bad, ref, bnd, f"{name} {store}->{out_fmt} fault {fault}")
    old = {"layernorm": lambda: _old_layernorm(fault, out_fmt), "add_layernorm_f32": lambda: _old_add_layernorm(fault, out_fmt),
           "layernorm_f32": lambda: _old_layernorm_f32(fault)}[name]()
    print(f"  old criterion of {name} ({out_fmt}) on its own operands, by width: " + ", ".join(f"{c}: {'accepted' if ok else 'rejected'}" for c, ok in old.items()))
    rejected = worst > 1.0
    if fault == "var_ex2" and store == "bf16":
        # |mean| / sigma = 294 is all that 8 significant bits allow: 4096 squares of 18 bits still sum without a visible loss
        print(f"  bf16 rows: the bound {'rejects' if rejected else 'accepts'} it ({worst:.3f}) - the f16 and fp32 rows are where it shows")
        return
    assert rejected, f"the per-element bound must reject {fault}"
    if fault == "var_ex2":
        assert int(op["profile"][place[0]]) == 1, "E[x^2] - mean^2 shows on the offset rows"
    # the fp32 kernel's own test is an fp32-ulp criterion: it sees the eps and variance faults; its gap is the ladder
    if fault in GAP and (name != "layernorm_f32" or fault == "ladder_off_by_one"):
        assert all(old.values()), f"the existing criterion was expected to accept {fault}: {old}"


def test_statistics_bound_rejects_the_variance_faults():
    """eps dropped / 1e-6 / outside the root and C - 1 in rstd itself, on the eps-dominant and plain rows."""
    op = X.rows_operands(131, 520, "bf16", "cycle", seed=2)
    mean, rstd = X.stats_reference(op["x"], op["eps"])
    var = (op["x"] - mean[:, None]).pow(2).mean(-1)
    br = X.stats_bound(op["x"], op["eps"], False)[1] * rstd
    for what, bad in (("eps dropped", 1 / torch.sqrt(var)), ("eps = 1e-6", 1 / torch.sqrt(var + 1e-6)), ("eps outside", 1 / (torch.sqrt(var) + 1e-5)),
                      ("C - 1", 1 / torch.sqrt(var * 520 / 519 + X.eps32(X.EPS)))):
        assert X.ratio(bad.float(), rstd, br, f"statistics with {what}")[0] > 1.0


def _old_head_post(fault, store):
    """tests/test_kernels_gpu.py::test_head_post_self on its own operands ((2, 4, 49, 2): N(0, 1) tokens, random angles): 1.5 u + 1e-5."""
    nseq, fps, L, heads = 2, 4, 49, 2
    seq_len, rows = fps * L, nseq * fps * L
    g = torch.Generator().manual_seed(1)
    x = torch.randn((rows, heads * 3 * 128), generator=g).to(X.FORMATS[store][0])
    w = torch.randn((128,), generator=g) * 0.2 + 1.0
    ang = torch.randn((nseq * fps, 64), generator=g) * 3.0
    rope = (ang.cos(), ang.sin())
    ref = X.head_reference(x, heads, 3, 0, w, rope, seq_len, L)[0]
    out = X.emulate_head(x, heads, 3, 0, w, rope, seq_len, L, store, fault=fault).double()
    return not bool(((out - ref).abs() > 1.5 * {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}[store] * ref.abs() + 1e-5).any())


@pytest.mark.parametrize("fault,store", [(f, s) for f in X.HEAD_FAULTS for s in STORES if f != "rounded_twice" or s == "bf16"])
def test_planted_head_split_faults_fail_the_bound(fault, store):
    nseq, fps, L, heads = HEAD_SHAPES[0]                 # frames of 49 tokens: the boundaries fall inside 16-token groups
    seq_len, rows = fps * L, nseq * fps * L
    assert L % 16 != 0
    x, prof = X.head_operands(rows, heads, 3, store, seed=L)
    wq, _ = X.head_weights(seed=L + 1)
    rope = X.rope_tables(nseq * fps, seed=L + 2)
    ref, terms = X.head_reference(x, heads, 3, 0, wq, rope, seq_len, L)
    bnd = X.head_bound(ref, terms, store, True)
    good = X.emulate_head(x, heads, 3, 0, wq, rope, seq_len, L, store)
    assert X.ratio(good, ref, bnd, f"head split {store} fault-free")[0] <= 1.0
    bad = X.emulate_head(x, heads, 3, 0, wq, rope, seq_len, L, store, fault=fault)
    worst, place = X.ratio(bad, ref, bnd, f"head split {store} fault {fault}")
    print(f"  old criterion of test_head_post_self ({store}) on its own operands: {'accepted' if _old_head_post(fault, store) else 'rejected'}")
    assert worst > 1.0, f"the per-element bound must reject {fault}"
    if fault == "frame_off_by_one":
        differs = ((bad.double() - good.double()).abs().amax((1, 3)) > 0).nonzero()[:, 1].unique().tolist()
        assert differs and all(s % L == 0 and s % 16 != 0 for s in differs), differs
