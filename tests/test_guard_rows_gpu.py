"""Guard bands of the row kernels (am_norm.hip, am_f32.hip): LayerNorm, its statistics forms, the fp32 residual stream, the fold
preparation - and of the head split (am_head_post, am_gemm_headpost_bf16) with a padded X.

The row kernels run four rows per workgroup and a row in chunks of 8 columns per lane: rows in {1, 3, 5, 1031} hit every remainder of
the row grouping, C in {8, 24, 264, 320, 4088, 4096} every per-lane `col < C` mask of every chunk-count instantiation (the suite
had multiples of 64 only), and 264 / 4088 the non-canonical statistics branch (C & 255).  Every output - and h32, updated in
place - sits in an arena of sentinels (tests/_guard.py); every value is compared with an fp64 statement at the bound the kernel's own
test uses; every result is compared bit for bit with the same call on plain tensors."""
import pytest
import torch
import torch.nn.functional as F

import test_f16_kernels_gpu as tf
import test_kernels_gpu as tk
from _guard import SENTINEL, Arena

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = tf.DTYPES
ROWS = [1, 3, 5, 1031]
COLS = [8, 24, 264, 320, 4088, 4096]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from actionmesh_amd import _lib
    _lib.lib()
    _lib.lib("f16")
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _ratio(what, err, bound):
    worst = float((err / bound).max())
    print(f"{what}: worst error / bound {worst:.3f}")
    assert worst <= 1.0, f"{what}: worst error / bound {worst:.3f}"
    return worst


def _stats_ref(x):
    x = x.double()
    return x.mean(-1), (x.var(-1, unbiased=False) + 1e-5).rsqrt()


def _check_stats(what, st, x):
    """test_row_stats_match_torch's tolerances against fp64 statistics: mean rtol 2e-6 + atol 2e-6, rstd rtol 5e-6."""
    mean, rstd = _stats_ref(x)
    _ratio(f"{what} mean", (st[:, 0].double() - mean).abs(), 2e-6 + 2e-6 * mean.abs())
    _ratio(f"{what} rstd", (st[:, 1].double() - rstd).abs(), 5e-6 * rstd)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_layernorm_and_row_stats_guards(dev, rows, C, dtype):
    """am_layernorm_bf16, am_layernorm_stats_bf16 and am_row_stats_bf16.  LayerNorm: 1.5 relative ulp + 1e-5 (test_layernorm);
    statistics: test_row_stats_match_torch's tolerances, and stats_out = row_stats of the rounded output, bit for bit.
    seen: layernorm 0.66 (both types); mean 0.04, rstd 0.03"""
    from actionmesh_amd import ops
    x = (tk._randn((rows, C), 1, dev) * 2.0 + 0.5).to(dtype)
    w = tk._randn((C,), 2, dev) * 0.2 + 1.0
    b = tk._randn((C,), 3, dev) * 0.2
    what = f"{dtype} {rows}x{C}"
    X = Arena.of(x)                                       # input: a read past the last row or column would meet a NaN
    Y, Y2 = Arena(rows, C, dtype, dev), Arena(rows, C, dtype, dev)
    S, S2 = Arena(rows, 2, torch.float32, dev), Arena(rows, 2, torch.float32, dev)
    ops.layernorm(X.view, w, b, 1e-5, out=Y.view)
    ops.layernorm(X.view, w, b, 1e-5, out=Y2.view, stats_out=S.view)
    ops.row_stats(X.view, out=S2.view)
    torch.cuda.synchronize()
    for nm, ar in (("x", X), ("y", Y), ("y (stats form)", Y2), ("stats_out", S), ("row_stats", S2)):
        ar.assert_untouched(f"{what}: {nm}")
    ref = F.layer_norm(x.double(), (C,), w.double(), b.double(), 1e-5)
    tf._close(Y.view, ref, 1.5, 1e-5, f"layernorm {what}", dtype=dtype)
    assert torch.equal(_bits(Y.view), _bits(Y2.view)) and torch.equal(_bits(Y.view), _bits(ops.layernorm(x, w, b, 1e-5)))
    _check_stats(f"row_stats {what}", S2.view, x)
    assert torch.equal(_bits(S2.view), _bits(ops.row_stats(x)))
    assert torch.equal(_bits(S.view), _bits(ops.row_stats(Y.view))), "stats_out are the statistics of the rounded output"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_add_layernorm_f32_guards(dev, rows, C, dtype):
    """am_add_layernorm_f32: h32 (in place) and z guarded, y an input arena.  test_add_layernorm_f32's statements: h exactly h + y
    (one fp32 add), z within 2^-7 (bf16) / 2^-10 (f16) of max|z| per element and rel-L2 < 2.5e-3 / 3.5e-4; the accumulate-only and
    LayerNorm-only forms.  seen: max-abs 0.48 (bf16) / 0.40 (f16) of the bound, rel-L2 0.76 / 0.72"""
    from actionmesh_amd import ops
    h = tk._randn((rows, C), 1, dev) * 3 + 2
    y = tk._randn((rows, C), 2, dev).to(dtype)
    w = tk._randn((C,), 3, dev).abs() * 0.5 + 0.5
    b = tk._randn((C,), 4, dev) * 0.3
    what = f"add_layernorm_f32 {dtype} {rows}x{C}"
    h_ref = h + y.float()
    z_ref = F.layer_norm(h_ref.double(), (C,), w.double(), b.double(), 1e-5)
    H, H2, H3, Yin, Z, Z3 = Arena.of(h), Arena.of(h), Arena.of(h_ref), Arena.of(y), Arena(rows, C, dtype, dev), Arena(rows, C, dtype, dev)
    ops.add_layernorm_f32(H.view, Yin.view, w, b, out=Z.view)
    assert ops.add_layernorm_f32(H2.view, Yin.view) is None                 # accumulate only
    ops.add_layernorm_f32(H3.view, None, w, b, out=Z3.view, dtype=dtype)     # LayerNorm only
    torch.cuda.synchronize()
    for nm, ar in (("h32", H), ("h32 (accumulate only)", H2), ("h32 (LayerNorm only)", H3), ("y", Yin), ("z", Z), ("z (LayerNorm only)", Z3)):
        ar.assert_untouched(f"{what}: {nm}")
    assert torch.equal(H.view, h_ref) and torch.equal(H2.view, h_ref) and torch.equal(H3.view, h_ref)
    tol = 2.0 ** (-7 if dtype == BF16 else -10) * float(z_ref.abs().max())
    mx = float((Z.view.double() - z_ref).abs().max()) / tol
    rl = tf._rel(Z.view, z_ref) / (2.5e-3 if dtype == BF16 else 3.5e-4)
    print(f"{what}: max-abs / bound {mx:.3f}, rel-L2 / bound {rl:.3f}")
    assert mx <= 1.0 and rl < 1.0
    assert torch.equal(_bits(Z.view), _bits(Z3.view))
    assert torch.equal(_bits(Z.view), _bits(ops.add_layernorm_f32(h.clone(), y, w, b)))


@pytest.mark.parametrize("C", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_layernorm_f32_guards(dev, rows, C):
    """am_layernorm_f32 at test_layernorm_f32_against_fp64's bound (4 fp32 ulp of |w| (|x| + |mean|) rstd + |b|).  seen: 0.68"""
    from actionmesh_amd import ops
    x = tk._randn((rows, C), 1, dev) * 3 + 0.5
    w, b = tk._randn((C,), 2, dev), tk._randn((C,), 3, dev)
    X, Y = Arena.of(x), Arena(rows, C, torch.float32, dev)
    ops.layernorm_f32(X.view, w, b, out=Y.view)
    torch.cuda.synchronize()
    X.assert_untouched("x")
    Y.assert_untouched("y")
    xd = x.double()
    mean, rstd = xd.mean(-1, keepdim=True), 1.0 / (xd.var(-1, unbiased=False, keepdim=True) + 1e-5).sqrt()
    ref = F.layer_norm(xd, (C,), None, None, 1e-5) * w.double() + b.double()
    _ratio(f"layernorm_f32 {rows}x{C}", (Y.view.double() - ref).abs(), 2.0 ** -21 * (w.double().abs() * (xd.abs() + mean.abs()) * rstd + b.double().abs()))
    assert torch.equal(_bits(Y.view), _bits(ops.layernorm_f32(x, w, b)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [264, 320, 4088, 4096])
@pytest.mark.parametrize("rows", [1, 257])
def test_row_stats_finalize_guards(dev, rows, C, dtype):
    """am_row_stats_finalize (both builds) on exact fp64-derived parts: the (mean, M2) of every 256-column slice of random rows, the
    last slice short when C % 256 != 0 - merged into (mean, rstd), against the fp64 statistics of the whole row at
    test_fold_under_large_row_means_and_outlier_channels' tolerances (mean rtol 2e-6 + atol 1e-6, rstd rtol 2e-5).
    seen: mean 0.09, rstd 0.01"""
    from actionmesh_amd import ops
    x = (tk._randn((rows, C), 5, dev) * 3.0 + 5.0).double()
    nparts = (C + 255) // 256
    part = torch.empty((rows, nparts, 2), dtype=torch.float64, device=dev)
    for j in range(nparts):
        sl = x[:, j * 256:(j + 1) * 256]
        part[:, j, 0] = sl.mean(-1)
        part[:, j, 1] = ((sl - sl.mean(-1, keepdim=True)) ** 2).sum(-1)
    P, S = Arena.flat_of(part.float()), Arena(rows, 2, torch.float32, dev)
    ops.row_stats_finalize(P.view, C, out=S.view, kind=dtype)
    torch.cuda.synchronize()
    P.assert_untouched("part")
    S.assert_untouched("stats")
    mean, rstd = _stats_ref(x)
    _ratio(f"finalize {dtype} {rows}x{C} mean", (S.view[:, 0].double() - mean).abs(), 1e-6 + 2e-6 * mean.abs())
    _ratio(f"finalize {dtype} {rows}x{C} rstd", (S.view[:, 1].double() - rstd).abs(), 2e-5 * rstd)
    assert torch.equal(_bits(S.view), _bits(ops.row_stats_finalize(part.float(), C, kind=dtype)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [64, 320])
@pytest.mark.parametrize("N", [1, 5])
def test_ln_fold_weight_guards(dev, N, K, dtype):
    """am_ln_fold_weight with wf, colsum and d guarded.  test_ln_fold_weight's statements against fp64: wf = the product rounded once
    (bf16: the same bits; f16: within 2^-11 of max|wf|), colsum and d at rtol 1e-5 + atol 1e-5.  seen: colsum below 0.001, d 0.004"""
    from actionmesh_amd import ops
    w = tk._randn((N, K), 3, dev, 0.05).to(dtype)
    gamma = tk._randn((K,), 4, dev).abs() * 0.5 + 0.5
    beta = tk._randn((K,), 5, dev) * 0.3
    bias = tk._randn((N,), 6, dev)
    Win = Arena.of(w)
    Wf, Cs, D = Arena(N, K, dtype, dev), Arena.flat((N,), torch.float32, dev), Arena.flat((N,), torch.float32, dev)
    ops.ln_fold_weight(Win.view, gamma, beta, bias, out=(Wf.view, Cs.view, D.view))
    torch.cuda.synchronize()
    for nm, ar in (("w", Win), ("wf", Wf), ("colsum", Cs), ("d", D)):
        ar.assert_untouched(f"ln_fold_weight {dtype} {N}x{K}: {nm}")
    want = (w.float() * gamma).to(dtype)                  # the kernel's definition: the fp32 product rounded to the type
    if dtype == BF16:
        assert torch.equal(_bits(Wf.view), _bits(want))
    else:
        want = (w.double() * gamma.double()).to(dtype)
        assert float((Wf.view.double() - want.double()).abs().max()) <= 2.0 ** -11 * float(want.double().abs().max())
    cs_ref, d_ref = Wf.view.double().sum(-1), w.double() @ beta.double() + bias.double()
    _ratio(f"ln_fold_weight {dtype} {N}x{K} colsum", (Cs.view.double() - cs_ref).abs(), 1e-5 + 1e-5 * cs_ref.abs())
    _ratio(f"ln_fold_weight {dtype} {N}x{K} d", (D.view.double() - d_ref).abs(), 1e-5 + 1e-5 * d_ref.abs())
    wf0, cs0, d0 = ops.ln_fold_weight(w, gamma, beta, bias)
    assert torch.equal(_bits(Wf.view), _bits(wf0)) and torch.equal(_bits(Cs.view), _bits(cs0)) and torch.equal(_bits(D.view), _bits(d0))


# ==========================================================================================================================================
# head split
# ==========================================================================================================================================
def _headpost_ref(x, heads, nparts, part, w, rope, seq_len, rpf):
    """test_kernels_gpu._headpost_ref in fp64: head split, qk-RMSNorm (eps 1e-6), RoPE by frame -> (nseq, H, seq_len, 128)."""
    rows = x.shape[0]
    xs = x.double().view(rows, heads, nparts, 128)[:, :, part]
    if w is not None:
        xs = xs * torch.rsqrt(xs.pow(2).mean(-1, keepdim=True) + 1e-6) * w.double()
    if rope is not None:
        fr = torch.arange(rows, device=x.device) // rpf
        c = rope[0].double()[fr].repeat_interleave(2, dim=-1)[:, None]
        s = rope[1].double()[fr].repeat_interleave(2, dim=-1)[:, None]
        xr, xi = xs.reshape(rows, heads, 64, 2).unbind(-1)
        xs = xs * c + torch.stack([-xi, xr], -1).flatten(2) * s
    return xs.view(rows // seq_len, seq_len, heads, 128).permute(0, 2, 1, 3)


def _operand_arenas(dev, dtype, kinds, nseq, heads, seq_len):
    """Q, K, V^T in flat guarded arenas.  The logical tensors start as zeros, not as sentinels: their pad rows / columns belong to the
    operand layout (Q zero padded, K pad rows and V^T pad columns zero) and the kernels rely on finite pads."""
    from actionmesh_amd import ops
    sq_pad, sk_pad = ops.round_up(seq_len, 256), ops.round_up(seq_len, 64)
    Q = Arena.flat((nseq, heads, sq_pad, 128), dtype, dev) if 0 in kinds else None
    K = Arena.flat((nseq, heads, sk_pad, 128), dtype, dev) if 1 in kinds else None
    Vt = Arena.flat((nseq, heads, 128, sk_pad), dtype, dev) if 2 in kinds else None
    for ar in (Q, K, Vt):
        if ar is not None:
            ar.view.zero_()
    return Q, K, Vt


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seq_len", [49, 64, 70])
@pytest.mark.parametrize("kinds", [(0, 1, 2), (0,), (1, 2)], ids=["qkv", "q", "kv"])
def test_head_post_guards_with_a_padded_x(dev, kinds, seq_len, dtype):
    """am_head_post reading X with ldx = width + 8 (gap columns: NaN) and writing Q, K, V^T into guarded arenas: two sequences of two
    heads; seq_len 49 (one partial 64-token block), 64 (exactly one), 70 (one full + one partial).  Q / K: 1.5 relative ulp + 1e-5
    (test_head_post_self); V^T: an exact gather in the perm16 order; pad rows / columns zero; the same bits as from a contiguous X.
    seen: Q 0.66, K 0.66"""
    from actionmesh_amd import ops
    nseq, heads = 2, 2
    rows, width = nseq * seq_len, heads * len(kinds) * 128
    x = tk._randn((rows, width), 1, dev).to(dtype)
    wq = tk._randn((128,), 2, dev) * 0.2 + 1.0
    wk = tk._randn((128,), 3, dev) * 0.2 + 1.0
    rope = None
    if len(kinds) == 3:                                   # the self-attention form carries RoPE, one frame per sequence here
        ang = tk._randn((nseq, 64), 4, dev) * 3.0
        rope = (ang.cos().contiguous(), ang.sin().contiguous())
    X = Arena.of(x, ld=width + 8)
    Q, K, Vt = _operand_arenas(dev, dtype, kinds, nseq, heads, seq_len)
    kw = dict(w_q=wq if 0 in kinds else None, w_k=wk if 1 in kinds else None, rope=rope)
    ops.head_post(X.view, heads, kinds, seq_len, seq_len, out_q=Q.view if Q else None, out_k=K.view if K else None,
                  out_vt=Vt.view if Vt else None, **kw)
    q0, k0, v0 = ops.head_post(x, heads, kinds, seq_len, seq_len, **kw)
    torch.cuda.synchronize()
    what = f"head_post {dtype} kinds {kinds} seq_len {seq_len}"
    for nm, ar, base in (("X", X, None), ("Q", Q, q0), ("K", K, k0), ("V^T", Vt, v0)):
        if ar is not None:
            ar.assert_untouched(f"{what}: {nm}")
            if base is not None:
                assert torch.equal(_bits(ar.view), _bits(base)), f"{what}: {nm} differs from the contiguous call"
    n = len(kinds)
    if Q:
        qr = _headpost_ref(x, heads, n, kinds.index(0), wq, rope, seq_len, seq_len)
        tf._close(Q.view[:, :, :seq_len], qr, 1.5, 1e-5, f"{what} Q", dtype=dtype)
        assert bool((Q.view[:, :, seq_len:] == 0).all())
    if K:
        kr = _headpost_ref(x, heads, n, kinds.index(1), wk, rope, seq_len, seq_len)
        tf._close(K.view[:, :, :seq_len], kr, 1.5, 1e-5, f"{what} K", dtype=dtype)
        assert bool((K.view[:, :, seq_len:] == 0).all())
    if Vt:
        vr = _headpost_ref(x, heads, n, kinds.index(2), None, None, seq_len, seq_len).float()
        sk_pad = Vt.view.shape[-1]
        vpad = torch.zeros((nseq, heads, sk_pad, 128), device=dev)
        vpad[:, :, :seq_len] = vr
        assert torch.equal(Vt.view.float(), vpad[:, :, ops.perm16_index(sk_pad, dev)].transpose(-1, -2).contiguous()), "V^T layout / perm16"


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_headpost_fused_guards(dev, dtype):
    """One fused launch: the two-sequence case of `_gemm_headpost_fused_case` (2 x 16 x 513 rows, two heads of q | k | v, qk-norm and
    RoPE; 32 remainder rows behind the 256-row grid) with K = 64.  Q, K, V^T and X are guarded; X starts as sentinels: the 32 tail
    rows go through it, and nothing else of X may change.  (c) every byte of Q, K, V^T equals am_gemm_bf16 + am_head_post on plain
    tensors; (b) that pair against fp64 in its two steps: the linear at the GEMM bound (seen: bf16 0.80, f16 0.44), Q / K of the valid
    tokens against the fp64 head split of the rounded linear at head_post's 1.5 relative ulp + 1e-5 (seen: 0.66)"""
    from actionmesh_amd import ops
    heads, kinds, T, Lr, B, Cw = 2, (0, 1, 2), 16, 513, 2, 64
    seq_len, rows, N = T * Lr, B * T * Lr, heads * 3 * 128
    a = tk._randn((rows, Cw), 1, dev).to(dtype)
    w = tk._randn((N, Cw), 2, dev, Cw ** -0.5).to(dtype)
    wq = tk._randn((128,), 3, dev) * 0.2 + 1.0
    wk = tk._randn((128,), 4, dev) * 0.2 + 1.0
    ang = torch.arange(B * T, device=dev)[:, None].float() * (10000.0 ** (-torch.arange(64, device=dev).float() * 2 / 128))[None]
    rope = (torch.cos(ang).contiguous(), torch.sin(ang).contiguous())
    kw = dict(w_q=wq, w_k=wk, rope=rope)
    x0 = ops.gemm(a, w)
    q0, k0, v0 = ops.head_post(x0, heads, kinds, seq_len, Lr, **kw)
    A, W = Arena.of(a), Arena.of(w)
    X = Arena(rows, N, dtype, dev)
    Q, K, Vt = _operand_arenas(dev, dtype, kinds, B, heads, seq_len)
    ops.gemm_head_post(A.view, W.view, heads, kinds, seq_len, Lr, out_q=Q.view, out_k=K.view, out_vt=Vt.view, x=X.view, **kw)
    torch.cuda.synchronize()
    for nm, ar, base in (("a", A, None), ("w", W, None), ("X", X, None), ("Q", Q, q0), ("K", K, k0), ("V^T", Vt, v0)):
        ar.assert_untouched(f"fused {dtype}: {nm}")
        if base is not None:
            bad = _bits(ar.view) != _bits(base)
            assert not bool(bad.any()), f"fused {dtype}: {nm} differs in {int(bad.sum())} elements, first at {bad.nonzero()[0].tolist()}"
    tail = rows % 256
    assert tail == 32
    xb = _bits(X.view)
    assert bool((xb[:rows - tail] == SENTINEL[dtype]).all()), "rows of X in front of the tail were written"
    assert torch.equal(xb[rows - tail:], _bits(x0[rows - tail:])), "the tail rows of X are the linear's output"
    # the un-fused pair itself against fp64: the linear at the GEMM bound, the head split of that linear at head_post's
    ref, lin = tf._gemm_ref(a, w, None, None, False)
    if dtype == F16:
        assert tf._report(f"fused {dtype}: linear", (x0.double() - ref).abs(), tf._gemm_bound(ref, lin)) <= 1.0
    else:
        tf._close(x0, ref, 2.0, 2e-3, f"fused {dtype}: linear", mag=lin.abs(), dtype=BF16)
    qr = _headpost_ref(x0, heads, 3, 0, wq, rope, seq_len, Lr)
    kr = _headpost_ref(x0, heads, 3, 1, wk, rope, seq_len, Lr)
    tf._close(Q.view[:, :, :seq_len], qr, 1.5, 1e-5, f"fused {dtype}: Q", dtype=dtype)
    tf._close(K.view[:, :, :seq_len], kr, 1.5, 1e-5, f"fused {dtype}: K", dtype=dtype)
