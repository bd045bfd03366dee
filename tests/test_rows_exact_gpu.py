"""Every row kernel, element by element, on exactly normalisable rows (GPU): LayerNorm and its statistics forms, the fp32 residual
stream, the fp32 LayerNorm, the producer's row parts and their merge, the head split with qk-RMSNorm and RoPE - alone and as the QKV
linear's fused epilogue - and the fold preparation, in the bf16 and the f16 build.

tests/_rows_exact.py: a row is m + s d with sum d = 0 and sum d^2 = 3 C, so every fp32 sum of the row and of its squared deviations
is exact in any order, and what a correct kernel may err by is counted from its source: half a spacing of the output at the fp64
reference plus a few 2^-24 of the terms.  No constant is fitted.  tests/test_rows_exact_cpu.py shows what this rejects and the
random-row tests accept.  Shapes: rows in {5, 131} (both remainders of the four-row workgroup), widths on both sides of every switch
of the launch ladders, the widths with a masked last chunk, and the two-pass (C % 256 != 0) and canonical forms of the statistics.
Every case prints its worst error / bound; the module prints the worst per kernel and type when it ends."""
import functools

import numpy as np
import pytest
import torch

import _rows_exact as X

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float16, id="f16")]
SENTINEL = -3.0
SEEN = {}


def _seen(kernel, fmt, worst):
    SEEN[(kernel, fmt)] = max(SEEN.get((kernel, fmt), 0.0), worst)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from actionmesh_amd import _lib
    _lib.lib()
    _lib.lib("f16")
    yield torch.device("cuda:0")
    _rows.cache_clear()
    for (kernel, fmt), worst in sorted(SEEN.items()):
        print(f"exact rows, worst error / bound: {kernel} {fmt} {worst:.3f}")


@functools.lru_cache(maxsize=8)
def _rows(rows, C, fmt, mode):
    """Operands (checked against their own conditions), on the device; shared by the kernels of a shape."""
    return X.rows_operands(rows, C, fmt, mode, seed=rows + C, device="cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _oracle_stats(x, eps):
    """oracle/row_stats_oracle.py on the rows' exact values -> (mean, rstd, parts) as numpy float32."""
    from oracle import row_stats_oracle as RO
    return RO.row_stats(x.float().cpu().numpy(), eps=eps)


def _against_oracle(st, x, eps, what):
    """The canonical statistics against their numpy restatement: the mean bit for bit, rstd within 2 fp32 spacings (the device's rsqrt
    is not the correctly rounded 1 / sqrt) - the statement of test_canonical_row_statistics_against_the_numpy_restatement."""
    mean, rstd, _ = _oracle_stats(x, eps)
    st = st.cpu().numpy()
    assert np.array_equal(st[:, 0].view(np.uint32), mean.view(np.uint32)), f"{what}: mean differs from the canonical restatement"
    ulp = np.abs(st[:, 1].view(np.int32).astype(np.int64) - rstd.view(np.int32).astype(np.int64))
    assert int(ulp.max()) <= 2, f"{what}: rstd {int(ulp.max())} spacings from the canonical restatement"


# ---- LayerNorm and the row statistics -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", X.WIDTHS)
@pytest.mark.parametrize("rows", X.ROWS)
def test_layernorm_and_statistics_are_exact_to_their_roundings(dev, rows, C, dtype):
    """am_layernorm_bf16, am_layernorm_stats_bf16, am_row_stats_bf16.  The output within ln_bound of fp64; a constant row gives b;
    the statistics within stats_bound (the two-pass mean bit for bit); stats_out == row_stats(y) bit for bit at every width - C % 256
    != 0 is the two-pass branch of the statistics of the output; the canonical widths against oracle/row_stats_oracle.py.
    seen: layernorm 0.997 (both types: a value half a spacing from the reference); row_stats mean 0.11, rstd 0.37"""
    from actionmesh_amd import ops
    fmt = X.NAME[dtype]
    for call in ("cycle", "unit"):
        op = _rows(rows, C, fmt, call)
        x, eps = op["x"], op["eps"]
        x16 = x.to(dtype)
        what = f"{fmt} {rows}x{C} {call}"
        rs = ops.row_stats(x16, eps)
        rm, rr = X.stats_check(rs, x, eps, C % 256 == 0, f"row_stats {what}")
        _seen("row_stats mean", fmt, rm)
        _seen("row_stats rstd", fmt, rr)
        if C % 256 == 0:
            _against_oracle(rs, x, eps, f"row_stats {what}")
        for b_mode in X.B_MODES:
            w, b = X.weights(C, b_mode, seed=C, device=dev)
            ref, term = X.ln_reference(x, w, b, eps)
            out = ops.layernorm(x16, w, b, eps)
            _seen("layernorm", fmt, X.check(out, ref, X.ln_bound(ref, term, fmt), f"layernorm {what} b {b_mode}"))
            const = op["profile"] == 3
            assert torch.equal(out[const].double(), X.rnd(b.double(), fmt).expand(int(const.sum()), C)), f"{what}: a constant row gives b"
            st = torch.full((rows, 2), float("nan"), device=dev)
            out2 = ops.layernorm(x16, w, b, eps, stats_out=st)
            assert torch.equal(_bits(out2), _bits(out)), f"{what}: the statistics form writes another output"
            assert torch.equal(_bits(st), _bits(ops.row_stats(out, eps))), f"{what}: stats_out are not row_stats of the rounded output"
            if C % 256 == 0:
                mean_y, _, _ = _oracle_stats(out, eps)
                assert np.array_equal(st[:, 0].cpu().numpy().view(np.uint32), mean_y.view(np.uint32)), f"{what}: stats_out mean is not canonical"


@pytest.mark.parametrize("dtype", DTYPES)
def test_unit_rows_measure_the_device_rsqrt(dev, dtype):
    """s = 1/2 and eps = 0.25 through the API: var + eps = 1 exactly in the two-pass form, so rstd - 1 is the error of the device's
    rsqrtf at 1.0, which _rows_exact.RSQRT_ULPS takes with one spacing of margin.  The head split's eps goes through the API too:
    vectors of +-1/2 and +-3/2 with eps = 0.25 and weight 1 have r = rsqrtf(1), and Q must be x itself.
    seen: 0 spacings in both builds (rstd == 1.0f on every row); head split: q == x bit for bit"""
    from actionmesh_amd import ops
    fmt = X.NAME[dtype]
    worst = 0.0
    for rows in X.ROWS:
        for C in (24, 264, 520, 4088):
            op = _rows(rows, C, fmt, "unit")
            rs = ops.row_stats(op["x"].to(dtype), op["eps"])
            assert torch.equal(rs[:, 0].double(), op["m"])
            worst = max(worst, float(X.ulps_f32(rs[:, 1], torch.ones_like(rs[:, 1])).max()))
    print(f"device rsqrtf at 1.0 ({fmt} build): {worst:.2f} fp32 spacings from 1")
    assert worst + 1.0 <= X.RSQRT_ULPS, f"rsqrtf(1.0f) is {worst} spacings off: RSQRT_ULPS must be that plus one"
    # the head split: vectors of +-1/2, +-3/2 (mean square 3/4), eps = 0.25, weight 1: r = rsqrtf(1) and q = x r
    d = X.pattern(64, 128, seed=7).to(dev)
    xh = (0.5 * d).to(dtype)
    q, _, _ = ops.head_post(xh, 1, (0,), 64, 64, w_q=torch.ones(128, device=dev), eps=X.UNIT_EPS)
    off = float(X.ulps_f32(q[0, 0, :64].float() / xh.float(), torch.ones((64, 128), device=dev)).max())
    print(f"head split's rsqrtf at 1.0 ({fmt} build): q / x within {off:.2f} fp32 spacings of 1")
    assert torch.equal(q[0, 0, :64], xh)


# ---- the fp32 residual stream ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", X.WIDTHS)
@pytest.mark.parametrize("rows", X.ROWS)
def test_add_layernorm_f32_is_exact_to_its_roundings(dev, rows, C, dtype):
    """am_add_layernorm_f32: h (fp32) and y (16-bit) exact with h + y the fp32 rows of the design (offset 2047 s); the three forms.
    h after the call is h + y bit for bit; z within ln_bound; the LayerNorm-only form gives the same bits.
    seen: 0.997 (both types)"""
    from actionmesh_amd import ops
    fmt = X.NAME[dtype]
    for call in ("cycle", "unit"):
        op = _rows(rows, C, "f32", call)
        x, eps = op["x"], op["eps"]
        g = torch.Generator().manual_seed(rows + C)
        e = (torch.randint(1, 3, (rows, C), generator=g) * (torch.randint(0, 2, (rows, C), generator=g) * 2 - 1)).double().to(dev)
        y = e * op["s"][:, None]                                              # +-s, +-2 s
        h = x - y
        y16, h32, x32 = y.to(dtype), h.float(), x.float()
        assert torch.equal(y16.double(), y) and torch.equal(h32.double(), h) and torch.equal(x32.double(), x)
        w, b = X.weights(C, X.B_MODES[(rows + C // 8) % 3], seed=C, device=dev)
        ref, term = X.ln_reference(x, w, b, eps)
        what = f"add_layernorm_f32 -> {fmt} {rows}x{C} {call}"
        h1 = h32.clone()
        z = ops.add_layernorm_f32(h1, y16, w, b, eps)
        assert z.dtype == dtype and torch.equal(_bits(h1), _bits(x32)), f"{what}: h is not h + y"
        _seen("add_layernorm_f32", fmt, X.check(z, ref, X.ln_bound(ref, term, fmt), what))
        h2 = h32.clone()
        assert ops.add_layernorm_f32(h2, y16, eps=eps) is None and torch.equal(_bits(h2), _bits(x32)), f"{what}: accumulate only"
        h3 = x32.clone()
        z3 = ops.add_layernorm_f32(h3, None, w, b, eps, dtype=dtype)
        assert torch.equal(_bits(z3), _bits(z)) and torch.equal(_bits(h3), _bits(x32)), f"{what}: LayerNorm only"


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("C", X.WIDTHS_F32)
@pytest.mark.parametrize("rows", X.ROWS)
def test_layernorm_f32_is_exact_to_its_roundings(dev, rows, C, kind):
    """am_layernorm_f32 (in both builds): 4 columns per lane, NCH in {1, 2, 4, 8, 16} from ceil(C / 256) - both sides of every switch.
    seen: 0.83 (both builds)"""
    from actionmesh_amd import ops
    for call in ("cycle", "unit"):
        op = _rows(rows, C, "f32", call)
        x, eps = op["x"], op["eps"]
        for b_mode in X.B_MODES:
            w, b = X.weights(C, b_mode, seed=C, device=dev)
            ref, term = X.ln_reference(x, w, b, eps)
            out = ops.layernorm_f32(x.float(), w, b, eps, kind=kind)
            _seen("layernorm_f32", kind, X.check(out, ref, X.ln_bound(ref, term, "f32"), f"layernorm_f32 ({kind} build) {rows}x{C} {call} b {b_mode}"))


# ---- the producer's row parts and their merge -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [512, 520])
def test_row_parts_of_a_copying_gemm_and_their_merge(dev, N, dtype):
    """ops.gemm(..., ln_part=) with one-hot weight rows: the output IS the exact rows.  1300 rows (test_producer_row_parts' fewest
    with both producers: 1280 through the store loop, 20 through the read-back pass); N = 520 ends in a slice of 8 columns,
    row_part_kernel's two-pass tail.  The parts equal the fp64 (mean, M2) of their slices bit for bit; row_stats_finalize within
    stats_bound; at N = 512 it is row_stats of the output bit for bit, and the numpy restatement's.
    seen: mean 0.005, rstd 0.37 (both types)"""
    from actionmesh_amd import ops
    fmt = X.NAME[dtype]
    M, K = 1300, ops.round_up(N, 64)
    op = _rows(M, N, fmt, "cycle")
    x, eps = op["x"], op["eps"]
    a = torch.zeros((M, K), dtype=dtype, device=dev)
    a[:, :N] = x.to(dtype)
    w = torch.zeros((N, K), dtype=dtype, device=dev)
    w[torch.arange(N), torch.arange(N)] = 1.0
    nparts = (N + 255) // 256
    part = torch.full((M, nparts, 2), float("nan"), device=dev)
    out = ops.gemm(a, w, force_big=True, ln_part=part)
    assert torch.equal(_bits(out), _bits(x.to(dtype))), "a one-hot weight row copies its column"
    want, _ = X.slice_parts(x)
    bad = (part.double() != want).any(-1)
    assert not bool(bad.any()), f"{int(bad.sum())} (row, slice) parts differ from fp64, first {bad.nonzero()[0].tolist()}: {part[bad][0].tolist()} != {want[bad][0].tolist()}"
    st = ops.row_stats_finalize(part, N, eps, kind=dtype)
    rm, rr = X.stats_check(st, x, eps, True, f"row_stats_finalize {fmt} {M}x{N}")
    _seen("row_stats_finalize mean", fmt, rm)
    _seen("row_stats_finalize rstd", fmt, rr)
    if N % 256 == 0:
        assert torch.equal(_bits(st), _bits(ops.row_stats(out, eps))), "the finalised parts are not row_stats of the rows"
        _against_oracle(st, x, eps, f"row_stats_finalize {fmt}")
        _, _, oparts = _oracle_stats(x, eps)
        assert np.array_equal(part.cpu().numpy().view(np.uint32), oparts.view(np.uint32))


# ---- the head split -------------------------------------------------------------------------------------------------------------------
def _sentinels(nseq, heads, seq_len, kinds, dtype, dev, sq_pad=None):
    from actionmesh_amd import ops
    sq_pad, sk_pad = sq_pad or ops.round_up(seq_len, 256), ops.round_up(seq_len, 64)
    full = lambda *shape: torch.full(shape, SENTINEL, dtype=dtype, device=dev)
    return (full(nseq, heads, sq_pad, 128) if 0 in kinds else None, full(nseq, heads, sk_pad, 128) if 1 in kinds else None,
            full(nseq, heads, 128, sk_pad) if 2 in kinds else None)


def _check_head_outputs(outs, x, prof, heads, kinds, seq_len, rpf, wq, wk, rope, fmt, what):
    """Q and K against the fp64 statement (head_check), the pad rows of Q untouched and of K zero, V^T bit for bit with zero pads."""
    from actionmesh_amd import ops
    q, k, vt = outs
    worst = 0.0
    for part, kind in enumerate(kinds):
        if kind == 2:
            ref = X.vt_reference(x, heads, len(kinds), part, seq_len, vt.shape[-1], ops.perm16_index(vt.shape[-1], x.device))
            assert torch.equal(vt.double(), ref), f"{what}: V^T layout / perm16 / zero pad columns"
            continue
        o, w = (q, wq) if kind == 0 else (k, wk)
        ref, terms = X.head_reference(x, heads, len(kinds), part, w, rope, seq_len, rpf)
        worst = max(worst, X.head_check(o[:, :, :seq_len], ref, terms, fmt, w is not None, rope is not None, prof, f"{what} {'QK'[kind]}"))
        pad = o[:, :, seq_len:]
        assert bool((pad == (SENTINEL if kind == 0 else 0.0)).all()), f"{what}: the pad rows of {'QK'[kind]}"
    return worst


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kinds", [(0, 1, 2), (0,), (1, 2)])
@pytest.mark.parametrize("nseq,frames_per_seq,L,heads", [(2, 2, 49, 1), (1, 1, 130, 3)])
def test_head_post_is_exact_to_its_roundings(dev, nseq, frames_per_seq, L, heads, kinds, dtype):
    """am_head_post with and without qk-RMSNorm, with and without RoPE.  Frames of 49 tokens: the frame boundaries fall inside 16-token
    groups, frames 1 .. 3 carry the pinned rotations; 130 tokens: three 64-token blocks, the last with 2 tokens.  Vectors of zeros give
    zeros, vectors far below eps stay inside the bound; without the norm the output is the rounded fp64 value bit for bit.
    seen: bf16 0.999, f16 0.995"""
    from actionmesh_amd import ops
    fmt = X.NAME[dtype]
    seq_len, rows = frames_per_seq * L, nseq * frames_per_seq * L
    x, prof = X.head_operands(rows, heads, len(kinds), fmt, seed=L + len(kinds), device=dev)
    wq, wk = X.head_weights(seed=L + 1, device=dev)
    tables = X.rope_tables(nseq * frames_per_seq, seed=L + 2, device=dev)
    for norm in (True, False):
        for rope in (tables, None):
            outs = _sentinels(nseq, heads, seq_len, kinds, dtype, dev)
            a, b = (wq, wk) if norm else (None, None)
            ops.head_post(x.to(dtype), heads, kinds, seq_len, L, w_q=a, w_k=b, rope=rope, out_q=outs[0], out_k=outs[1], out_vt=outs[2])
            what = f"head_post {fmt} ({nseq}, {frames_per_seq}, {L}, {heads}) kinds {kinds} norm={norm} rope={rope is not None}"
            _seen("head_post", fmt, _check_head_outputs(outs, x, prof, heads, kinds, seq_len, L, a, b, rope, fmt, what))


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_qkv_epilogue_is_head_post_of_the_exact_rows(dev, dtype):
    """ops.gemm_head_post at the smallest shape that takes the fused path (the "self_qkv_tail_and_straddle" geometry of
    test_gemm_headpost_fused_is_bit_identical: two sequences of 16 frames of 513 tokens, 64 row tiles and 32 tail rows, two heads) with
    one-hot weights: the linear's output is the exact token rows, tiny and zero vectors included.  Bit for bit head_post of those rows,
    which is itself checked against the bound.
    seen: bf16 0.999, f16 0.995 (the values of head_post: the same bits)"""
    from actionmesh_amd import ops
    fmt = X.NAME[dtype]
    heads, kinds, T, L, B = 2, (0, 1, 2), 16, 513, 2
    seq_len, rows, N = T * L, B * T * L, heads * 3 * 128
    x, prof = X.head_operands(rows, heads, 3, fmt, seed=11, device=dev)
    x16 = x.to(dtype)
    w = torch.eye(N, dtype=dtype, device=dev)
    assert torch.equal(_bits(ops.gemm(x16, w)), _bits(x16)), "a one-hot weight row copies its column"
    wq, wk = X.head_weights(seed=12, device=dev)
    rope = X.rope_tables(B * T, seed=13, device=dev)
    plain = _sentinels(B, heads, seq_len, kinds, dtype, dev)
    ops.head_post(x16, heads, kinds, seq_len, L, w_q=wq, w_k=wk, rope=rope, out_q=plain[0], out_k=plain[1], out_vt=plain[2])
    fused = _sentinels(B, heads, seq_len, kinds, dtype, dev)
    ops.gemm_head_post(x16, w, heads, kinds, seq_len, L, w_q=wq, w_k=wk, rope=rope, out_q=fused[0], out_k=fused[1], out_vt=fused[2])
    torch.cuda.synchronize()
    for nm, r, f in zip(("Q", "K", "V^T"), plain, fused):
        bad = _bits(r) != _bits(f)
        assert not bool(bad.any()), f"{nm} differs in {int(bad.sum())} elements, first at {bad.nonzero()[0].tolist()}"
    _seen("fused QKV epilogue", fmt, _check_head_outputs(fused, x, prof, heads, kinds, seq_len, L, wq, wk, rope, fmt, f"fused QKV epilogue {fmt}"))


# ---- the fold preparation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [8, 64, 72, 320])
@pytest.mark.parametrize("N", [1, 5])
def test_ln_fold_weight_is_exact(dev, N, K, dtype):
    """am_ln_fold_weight on operands whose products and sums are exact: wf, colsum and d equal the fp64 values bit for bit, with and
    without bias.  One wave per output row, 64 columns per trip: K = 8 leaves 56 lanes idle, 72 and 320 end in a partial trip."""
    from actionmesh_amd import ops
    W, gamma, beta, bias = X.fold_operands(N, K, seed=N + K, device=dev)
    for bs in (bias, None):
        wf, colsum, d = ops.ln_fold_weight(W.to(dtype), gamma.float(), beta.float(), None if bs is None else bs.float())
        rwf, rcs, rd = X.fold_reference(W, gamma, beta, bs)
        assert wf.dtype == dtype and torch.equal(wf.double(), rwf), "wf is not W gamma"
        assert torch.equal(colsum.double(), rcs), "colsum is not the row sum of wf"
        assert torch.equal(d.double(), rd), "d is not W beta + bias"
