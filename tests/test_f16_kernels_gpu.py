"""Kernel-level tests of the float16 build (libactionmesh_amd_f16.so, -DAM_F16) and of IEEE half's range edges.

The float16 library is not "the bf16 code with another type": it has its own MFMA opcodes, v_dot2c_f32_f16 row sums in the 4x64 attention,
no GELU table, the exact running-max attention instead of the lazy re-base, compiler-generated _Float16 conversions - and a format with 5
exponent bits (subnormal below 2^-14, nothing below 2^-25, infinite from 65520 up).  Three kinds of test:

A. float16 twins of the bf16 kernel-route tests of test_kernels_gpu.py (forced GEMM tiles, row maps, head_post, fused QKV, the forced
   attention geometries, two-pass, key coverage), at the project's own float16 tolerances.
B. exact-arithmetic GEMMs (both dtypes): operands made of small integers times powers of two, so that every product and every partial sum
   is exact in fp32 in any order and the expected output is known to the BIT - subnormal operands, subnormal outputs, overflow to +-inf.
C. softmax whose probabilities lie in half's subnormal range (keys 16 .. 24 octaves under the row maximum, carrying up to half of the
   softmax mass), and the norm / elementwise kernels at the edges of the range.

Every reference is computed from the SAME 16-bit operands in fp64 (or fp32 where the bf16 twin does), rounded where the kernel rounds.
Every test prints its worst error over its bound."""
import math

import pytest
import torch
import torch.nn.functional as F

import test_kernels_gpu as tk          # the tests directory is on sys.path (pytest rootdir / conftest)

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = [pytest.param(F16, id="f16"), pytest.param(BF16, id="bf16")]
U = {F16: 2.0 ** -11, BF16: 2.0 ** -8}       # largest relative error of one round-to-nearest to the type (half a spacing)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from actionmesh_amd import _lib
    _lib.lib("f16")   # fail loudly if the float16 library is missing
    return torch.device("cuda:0")


def _randn(shape, seed, dev, scale=1.0):
    return tk._randn(shape, seed, dev, scale)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _report(what, err, bound):
    """Print and return the worst error / bound over all elements (no outlier allowance anywhere in this module)."""
    worst = float((err / bound).max())
    print(f"{what}: worst error / bound {worst:.3f}")
    return worst


def _close(out, ref, ulps, atol, what, mag=None, dtype=F16):
    """The bf16 tests' `_close` with the rounding unit of `dtype`: |out - ref| <= ulps * U * max(|ref|, mag) + atol, every element."""
    ref = ref.double()
    scale = ref.abs() if mag is None else torch.maximum(ref.abs(), mag.double())
    worst = _report(what, (out.double() - ref).abs(), ulps * U[dtype] * scale + atol)
    assert worst <= 1.0, f"{what}: worst error / bound {worst:.3f}"
    return worst


# ==========================================================================================================================================
# A.  GEMM routes
# ==========================================================================================================================================
ROUTES = {"dispatch": {}, "small": dict(force_small=True), "big": dict(force_big=True), "lockstep": dict(force_big=True, legacy=True)}


def _gemm_ref(a, w, bias, res, gelu):
    """fp64 statement of the GEMM from the same 16-bit operands, rounded where the kernel rounds: the linear (+ fp32 bias) once, GELU of the
    rounded linear once, the residual added to the rounded value and rounded.  Returns (ref, rounded linear), fp64."""
    dt = a.dtype
    ref = a.double() @ w.double().T
    if bias is not None:
        ref = ref + bias.double()
    lin = ref.float().to(dt).double()
    ref = lin
    if gelu:
        ref = F.gelu(ref.float()).to(dt).double()
    if res is not None:
        ref = (ref + res.double()).float().to(dt).double()
    return ref, lin


def _gemm_bound(ref, lin):
    """test_gemm_f16's bound: 2 half ulp (2^-10 relative) of max(|value|, |rounded linear|) + 3e-4 for the fp32 accumulation noise."""
    return 2.0 * torch.maximum(ref.abs(), lin.abs()) * 2.0 ** -10 + 3e-4


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


GEMM_SHAPES = [(37, 128, 64), (300, 256, 128), (1000, 384, 256), (4097, 1024, 1024), (2500, 3072, 512), (256, 256, 4096), (5000, 520, 320),
               (33792 + 32, 1024, 256)]


@pytest.mark.parametrize("mode", ["plain", "bias", "bias_gelu", "bias_res"])
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_routes_f16(dev, M, N, K, mode):
    """Every GEMM kernel of the float16 build on the same problem: the product dispatch, the 128x128 tile, the 256x256 ping-pong tile and
    its lockstep loop.  Under force_big 4097 rows end in gemm_tail_kernel (M > 2048, remainder 1) and 2500 rows in a partial 256-row
    tile (196); 33 824 x 1024 is the product dispatch's own big path + tail kernel (132 x 4 tiles >= 192) and runs that route only.
    Bound: test_gemm_f16's (seen: 0.89 of it in the GELU mode, 0.81 elsewhere; rel-L2 <= 2.0e-5).  Ping-pong against lockstep: the same
    products summed in another order, i.e. linears one half spacing apart at most (2^-10 |linear|); GELU' <= 1.13 carries that to the
    activation, and a second rounding (activation / residual add) can flip once more: 2^-10 (1.13 |linear| + |value|) + the 3e-4 floor
    (seen: 0 - the two loops are bit-equal in all 28 cases)"""
    from actionmesh_amd import ops
    a = _randn((M, K), 1, dev).half()
    w = _randn((N, K), 2, dev, 1.0 / math.sqrt(K)).half()
    bias = _randn((N,), 3, dev, 0.5) if mode != "plain" else None
    res = _randn((M, N), 4, dev).half() if mode == "bias_res" else None
    kw = dict(bias=bias, residual=res, gelu=(mode == "bias_gelu"))
    ref, lin = _gemm_ref(a, w, bias, res, kw["gelu"])
    bound = _gemm_bound(ref, lin)
    routes = ["dispatch"] if M > 30000 else list(ROUTES)
    outs = {}
    for r in routes:
        out = ops.gemm(a, w, **kw, **ROUTES[r])
        again = ops.gemm(a, w, **kw, **ROUTES[r])
        torch.cuda.synchronize()
        assert out.dtype == F16
        worst = _report(f"f16 gemm {M}x{N}x{K} {mode} {r}", (out.double() - ref).abs(), bound)
        rl = _rel(out, ref)
        print(f"    rel-L2 {rl:.2e}")
        assert worst <= 1.0 and rl < 5e-4, (r, worst, rl)
        assert torch.equal(_bits(out), _bits(again)), f"{r}: run-to-run bits"
        outs[r] = out
    if "lockstep" in outs:
        post = ref.abs() if mode in ("bias_gelu", "bias_res") else 0.0
        worst = _report(f"f16 gemm {M}x{N}x{K} {mode} ping-pong vs lockstep", (outs["big"].double() - outs["lockstep"].double()).abs(),
                        2.0 ** -10 * (1.13 * lin.abs() + post) + 3e-4)
        assert worst <= 1.0


def _map_case(dev, dtype, frames, N=328):
    """The operands of test_gemm256_split_a_row_maps_and_tails: split A, a_map and c_map (rows 1 .. 48 of every 49-row frame), in-place
    residual, M and N tails.  Asserts that row 0 of every frame is untouched; returns (written rows, ref, rounded linear, residual rows)."""
    from actionmesh_amd import ops
    G, L = 48, 49
    M, K1, K2 = frames * G, 128, 64
    a1 = _randn((frames * L, K1), 1, dev).to(dtype)
    a2 = _randn((frames * L, K2), 2, dev).to(dtype)
    w = _randn((N, K1 + K2), 3, dev, 0.07).to(dtype)
    bias = _randn((N,), 4, dev, 0.5).to(dtype).float()
    res = _randn((frames * L, N), 5, dev).to(dtype)
    dst = res.clone()
    ops.gemm(a1, w, bias=bias, a2=a2, residual=dst, out=dst, a_map=(G, L, 1), c_map=(G, L, 1), M=M, force_big=True)
    torch.cuda.synchronize()
    cat = torch.cat([a1, a2], 1).view(frames, L, K1 + K2)[:, 1:].reshape(M, K1 + K2)
    r3 = res.view(frames, L, N)
    ref, lin = _gemm_ref(cat, w, bias, r3[:, 1:].reshape(M, N), False)
    got = dst.view(frames, L, N)
    assert torch.equal(_bits(got[:, 0]), _bits(r3[:, 0])), "row 0 of every frame must be untouched"
    return got[:, 1:].reshape(M, N), ref, lin, r3[:, 1:].reshape(M, N)


def test_gemm256_split_a_row_maps_and_tails_f16(dev):
    """float16 twin of test_gemm256_split_a_row_maps_and_tails (30 frames: M = 1440, tail 160 of 256; N = 328).  seen: 0.57"""
    got, ref, lin, _ = _map_case(dev, F16, 30)
    assert _report("f16 gemm256 maps", (got.double() - ref).abs(), _gemm_bound(ref, lin)) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm256_row_maps_with_a_remainder_behind_the_grid(dev, dtype):
    """43 frames x 48 rows = 2064 = 8 x 256 + 16 under force_big: M > 2048 with a remainder <= 128 cuts the last 16 rows off the 256-row
    grid, and because the row maps are not the identity launch_tail must hand them to the 128x128 tile, not to gemm_tail_kernel (which
    knows no row maps).  No other test reaches that branch.  float16: the GEMM bound (seen: 0.57); bf16: the bound of its 30-frame
    twin (2 ulp + 4e-3; seen: 0.66)"""
    got, ref, lin, res = _map_case(dev, dtype, 43)
    if dtype == F16:
        assert _report("f16 gemm256 maps + remainder", (got.double() - ref).abs(), _gemm_bound(ref, lin)) <= 1.0
    else:
        _close(got, lin + res.double(), 2.0, 4e-3, "bf16 gemm256 maps + remainder", mag=torch.maximum(lin.abs(), res.double().abs()), dtype=BF16)


def test_gemm_split_a_and_row_maps_f16(dev):
    """float16 twin of test_gemm_split_a_and_row_maps (the 128x128 tile).  seen: split-A 0.37, c_map 0.25, a_map 0.04"""
    from actionmesh_amd import ops
    M, N, K1, K2 = 517, 256, 128, 192
    a1 = _randn((M, K1), 1, dev).half()
    a2 = _randn((M, K2), 2, dev).half()
    w = _randn((N, K1 + K2), 3, dev, 0.05).half()
    bias = _randn((N,), 4, dev, 0.5)
    out = ops.gemm(a1, w, bias=bias, a2=a2)
    ref, lin = _gemm_ref(torch.cat([a1, a2], 1), w, bias, None, False)
    assert _report("f16 split-A gemm", (out.double() - ref).abs(), _gemm_bound(ref, lin)) <= 1.0
    frames, G, L = 5, 48, 49
    a = _randn((frames * G, 64), 5, dev).half()
    w = _randn((256, 64), 6, dev, 0.1).half()
    dst = torch.full((frames * L, 256), 7.0, dtype=F16, device=dev)
    ops.gemm(a, w, out=dst, c_map=(G, L, 1))
    ref, lin = _gemm_ref(a, w, None, None, False)
    got = dst.view(frames, L, 256)
    assert _report("f16 c_map rows", (got[:, 1:].reshape(-1, 256).double() - ref).abs(), _gemm_bound(ref, lin)) <= 1.0
    assert bool((got[:, 0] == 7.0).all()), "row 0 of every frame must be untouched"
    src = _randn((frames * L, 128), 8, dev).half()
    w2 = _randn((64, 128), 9, dev, 0.1).half()
    out2 = ops.gemm(src, w2, a_map=(G, L, 1), M=frames * G)
    ref2, lin2 = _gemm_ref(src.view(frames, L, 128)[:, 1:].reshape(-1, 128), w2, None, None, False)
    assert _report("f16 a_map rows", (out2.double() - ref2).abs(), _gemm_bound(ref2, lin2)) <= 1.0


def test_gemm_in_place_residual_f16(dev):
    """seen: 0.41"""
    from actionmesh_amd import ops
    M, N, K = 700, 256, 256
    a = _randn((M, K), 1, dev).half()
    w = _randn((N, K), 2, dev, 0.06).half()
    h = _randn((M, N), 3, dev).half()
    ref, lin = _gemm_ref(a, w, None, h, False)
    ops.gemm(a, w, residual=h, out=h)
    assert _report("f16 in-place residual", (h.double() - ref).abs(), _gemm_bound(ref, lin)) <= 1.0


@pytest.mark.parametrize("scale,ln", [(1.0, False), (3.5, False), (0.02, False), (1.0, True)])
def test_gelu_has_one_form_f16(dev, scale, ln):
    """The float16 build has no GELU table (gelu_table() returns nullptr): gelu_table=True and gelu_table=False must both take the
    arithmetic epilogue and give the same bits, on the inputs of test_gelu_table_is_bit_identical."""
    from actionmesh_amd import ops
    M, N, K = 2048 + 256, 1024, 512
    a = _randn((M, K), 11, dev, scale).half()
    a[5] = 0
    a[300:310] = 0
    w = _randn((N, K), 12, dev, K ** -0.5).half()
    bias = _randn((N,), 13, dev, 0.5 * scale)
    bias[:8] = torch.tensor([0.0, -0.0, 9.0, -9.0, 300.0, -300.0, 1e-6, -1e-6], device=dev)
    kw = {}
    if ln:
        gamma = torch.rand(K, device=dev) + 0.5
        beta = torch.randn(K, device=dev) * 0.2
        wf, colsum, d = ops.ln_fold_weight(w, gamma, beta, bias)
        w, bias, kw = wf, d, dict(ln=(ops.row_stats(a), colsum))
    tab = ops.gemm(a, w, bias=bias, gelu=True, force_big=True, **kw)
    ari = ops.gemm(a, w, bias=bias, gelu=True, force_big=True, gelu_table=False, **kw)
    torch.cuda.synchronize()
    assert torch.equal(_bits(tab), _bits(ari)), f"{int((_bits(tab) != _bits(ari)).sum())} elements differ"
    pre = ops.gemm(a, w, bias=bias, force_big=True, **kw).float()
    ref = F.gelu(pre)
    worst = float((tab.float() - ref).abs().max()) / (2.0 ** -11 * max(1.0, float(ref.abs().max())))
    print(f"f16 gelu scale {scale} ln {ln}: worst error / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_refuses_folded_layernorm_over_row_map_on_the_256_tile(dev, dtype):
    """A folded LayerNorm over a row-mapped A is the 128x128 tile's job (it indexes the statistics by the mapped A row; the 256x256
    tile indexes them by output row).  N < 256 used to be accepted on the assumption that the 128 tile runs - but force_big sends any
    N to the 256 tile: that combination is refused with AM_ERR_INVALID (-1); with force_small as well the 128 tile runs and it is accepted."""
    from actionmesh_amd import ops
    frames, G, L, K, N = 6, 48, 49, 128, 64
    src = _randn((frames * L, K), 1, dev).to(dtype)
    w = _randn((N, K), 2, dev, 0.1).to(dtype)
    gamma, beta = torch.rand(K, device=dev) + 0.5, torch.randn(K, device=dev) * 0.2
    wf, colsum, d = ops.ln_fold_weight(w, gamma, beta, None)
    kw = dict(bias=d, ln=(ops.row_stats(src), colsum), a_map=(G, L, 1), M=frames * G)
    with pytest.raises(RuntimeError, match=r"status -1"):
        ops.gemm(src, wf, force_big=True, **kw)
    ok = ops.gemm(src, wf, **kw)
    both = ops.gemm(src, wf, force_big=True, force_small=True, **kw)
    assert torch.equal(_bits(ok), _bits(both))
    x = src.view(frames, L, K)[:, 1:].reshape(-1, K).float()
    ref = F.layer_norm(x, (K,), gamma, beta, 1e-5).to(dtype).float() @ w.float().T
    # the folded form differs from LayerNorm-then-linear by the 16-bit rounding of the normalised activation (ops.ln_fold_weight):
    # a sanity bound only (wrong statistics rows are off by O(1)); the fold's own tolerances are test_ln_fold_gpu.py's
    err = float((ok.float() - ref).abs().max())
    print(f"{dtype} folded LayerNorm over a_map (128 tile): max abs err {err:.2e}, ref max {float(ref.abs().max()):.2f}")
    assert err <= 16 * U[dtype] * float(ref.abs().max()) + 1e-2


# ==========================================================================================================================================
# A.  LayerNorm, head_post, the fused QKV projection
# ==========================================================================================================================================
@pytest.mark.parametrize("rows,C", [(50, 256), (4097, 1024), (1031, 2048), (64, 4096)])
def test_layernorm_f16(dev, rows, C):
    """seen: 0.66"""
    from actionmesh_amd import ops
    x = (_randn((rows, C), 1, dev) * 2.0 + 0.5).half()
    w = _randn((C,), 2, dev) * 0.2 + 1.0
    b = _randn((C,), 3, dev) * 0.2
    out = ops.layernorm(x, w, b, 1e-5)
    ref = F.layer_norm(x.double(), (C,), w.double(), b.double(), 1e-5)
    _close(out, ref, 1.5, 1e-5, f"f16 layernorm {rows}x{C}")


@pytest.mark.parametrize("nseq,frames_per_seq,L,heads", [(2, 4, 49, 2), (1, 3, 70, 3), (6, 1, 130, 2)])
def test_head_post_self_f16(dev, nseq, frames_per_seq, L, heads):
    """seen: Q 0.66, K 0.66"""
    from actionmesh_amd import ops
    seq_len = frames_per_seq * L
    rows = nseq * seq_len
    x = _randn((rows, heads * 3 * 128), 1, dev).half()
    wq = _randn((128,), 2, dev) * 0.2 + 1.0
    wk = _randn((128,), 3, dev) * 0.2 + 1.0
    ang = _randn((nseq * frames_per_seq, 64), 4, dev) * 3.0
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    q, k, vt = ops.head_post(x, heads, (0, 1, 2), seq_len, L, w_q=wq, w_k=wk, rope=(cos, sin))
    torch.cuda.synchronize()
    assert q.dtype == F16
    qr = tk._headpost_ref(x, heads, 3, 0, wq, (cos, sin), seq_len, L)
    kr = tk._headpost_ref(x, heads, 3, 1, wk, (cos, sin), seq_len, L)
    vr = tk._headpost_ref(x, heads, 3, 2, None, None, seq_len, L)
    _close(q[:, :, :seq_len], qr, 1.5, 1e-5, "f16 head_post Q")
    _close(k[:, :, :seq_len], kr, 1.5, 1e-5, "f16 head_post K")
    assert bool((q[:, :, seq_len:] == 0).all()) and bool((k[:, :, seq_len:] == 0).all())
    sk_pad = vt.shape[-1]
    idx = ops.perm16_index(sk_pad, dev)
    vpad = torch.zeros((nseq, heads, sk_pad, 128), device=dev)
    vpad[:, :, :seq_len] = vr
    assert torch.equal(vt.float(), vpad[:, :, idx].transpose(-1, -2).contiguous()), "V^T layout / perm16"


def test_head_post_cross_f16(dev):
    """seen: Q 0.66, K 0.65"""
    from actionmesh_amd import ops
    heads, L, S, BT = 2, 49, 9, 5
    xq = _randn((BT * L, heads * 128), 1, dev).half()
    wq = _randn((128,), 2, dev) * 0.2 + 1.0
    q, _, _ = ops.head_post(xq, heads, (0,), L, L, w_q=wq)
    _close(q[:, :, :L], tk._headpost_ref(xq, heads, 1, 0, wq, None, L, L), 1.5, 1e-5, "f16 cross Q")
    assert bool((q[:, :, L:] == 0).all())
    xkv = _randn((BT * S, heads * 2 * 128), 3, dev).half()
    wk = _randn((128,), 4, dev) * 0.2 + 1.0
    _, k, vt = ops.head_post(xkv, heads, (1, 2), S, S, w_k=wk)
    _close(k[:, :, :S], tk._headpost_ref(xkv, heads, 2, 0, wk, None, S, S), 1.5, 1e-5, "f16 cross K")
    assert bool((k[:, :, S:] == 0).all())
    vr = tk._headpost_ref(xkv, heads, 2, 1, None, None, S, S)
    idx = ops.perm16_index(vt.shape[-1], dev)
    vpad = torch.zeros((BT, heads, vt.shape[-1], 128), device=dev)
    vpad[:, :, :S] = vr
    assert torch.equal(vt.float(), vpad[:, :, idx].transpose(-1, -2).contiguous())


@pytest.mark.parametrize("case", ["self_qkv_tail_and_straddle", "cross_q", "no_norm_no_rope", "misaligned_falls_back", "small_falls_back"])
def test_gemm_headpost_fused_is_bit_identical_f16(dev, case):
    """am_gemm_headpost_bf16 of the float16 build against am_gemm_bf16 + am_head_post: every byte (test_kernels_gpu.py)."""
    tk._gemm_headpost_fused_case(dev, case, dtype=F16)


# ==========================================================================================================================================
# A.  attention routes
# ==========================================================================================================================================
F16_ATTN_TOL = 2e-3       # the float16 rel-L2 of test_cross_attention_with_the_resident_key_stream


def _qkv(dev, nseq, H, sq, sk, dtype=F16):
    return (_randn((nseq, H, sq, 128), 1, dev).to(dtype), _randn((nseq, H, sk, 128), 2, dev).to(dtype), _randn((nseq, H, sk, 128), 3, dev).to(dtype))


@pytest.mark.parametrize("nseq,H,sq,sk,nchunks", [(1, 2, 300, 300, 1), (2, 2, 196, 196, 1), (5, 2, 49, 9, 1),
                                                  (3, 2, 70, 17, 1), (1, 1, 1000, 64, 1), (2, 2, 196, 196, 2),
                                                  (1, 2, 520, 1040, 4), (2, 8, 2049, 257, 1),
                                                  (1, 2, 2320, 4200, 1), (2, 1, 2305, 4224, 2), (1, 1, 2432, 4097, 1)])
def test_attention_routes_f16(dev, nseq, H, sq, sk, nchunks):
    """The shapes of test_attention under every dispatch code (product 0 / 8, 4x64 exact 28 / 60 / 68, 8-wave 90 / 98, two 4-wave
    workgroups 58, balanced 78).  seen: rel-L2 <= 3.6e-4 (0.18 of the tolerance)"""
    from actionmesh_amd import ops
    q, k, v = _qkv(dev, nseq, H, sq, sk)
    Q, K, Vt, skc = tk._layout(q, k, v, nchunks)
    assert Q.dtype == F16
    ref = tk._sdpa_ref(q, k, v).permute(0, 2, 1, 3).reshape(nseq * sq, H * 128)
    for defer in (0, 8, 28, 60, 68, 90, 98, 58, 78):
        out = ops.attention(Q, K, Vt, sq, skc, nchunks=nchunks, defer_log2=defer)
        torch.cuda.synchronize()
        assert out.dtype == F16
        r = tk._attn_close(out, ref, f"f16 attention defer={defer}", rel_tol=F16_ATTN_TOL)
        print(f"f16 attention {nseq}x{H}x{sq}x{sk}/{nchunks} defer={defer}: rel-L2 / tolerance {r / F16_ATTN_TOL:.3f}")


@pytest.mark.parametrize("defer", [0, 8])
@pytest.mark.parametrize("nseq,H,sq,skc,P", [(2, 2, 2320, 1100, 4), (1, 2, 2304, 1024, 2), (1, 1, 2432, 1030, 3)])
def test_attention_two_pass_matches_one_pass_f16(dev, nseq, H, sq, skc, P, defer):
    """float16 twin of test_attention_two_pass_matches_one_pass, with its sentinel checks.  seen: rel-L2 <= 3.6e-4"""
    from actionmesh_amd import ops
    q, k, v = _qkv(dev, nseq, H, sq, skc * P)
    Q, K, Vt, skc_ = tk._layout(q, k, v, P)
    assert skc_ == skc
    ref = tk._sdpa_ref(q, k, v).permute(0, 2, 1, 3).reshape(nseq * sq, H * 128)
    one = ops.attention(Q, K, Vt, sq, skc, nchunks=P, defer_log2=defer).float()
    tk._attn_close(one, ref, "one pass", rel_tol=F16_ATTN_TOL)
    state = torch.full((nseq * H, Q.shape[2], ops.STATE_LD), float("nan"), device=dev)
    for r in range(P):
        out = torch.full((nseq * sq, H * 128), 768.0, dtype=F16, device=dev)
        ops.attention(Q, K, Vt, sq, skc, out=out, nchunks=1, defer_log2=defer, rows=1, state_mode=1, state=state, chunk_first=r, chunk_total=P)
        assert (out.float() == 768.0).all(), "the first pass must not write the output"
        ops.attention(Q, K, Vt, sq, skc, out=out, nchunks=P - 1, defer_log2=defer, rows=1, state_mode=2, state=state,
                      chunk_first=(r + 1) % P, chunk_total=P)
        ops.attention(Q, K, Vt, sq, skc, out=out, nchunks=P, defer_log2=defer, rows=2)
        torch.cuda.synchronize()
        o = out.float()
        assert not (o == 768.0).any(), f"rank {r}: rows left unwritten"
        r1 = tk._attn_close(o, ref, f"rank {r} vs fp32 reference", rel_tol=F16_ATTN_TOL)
        r2 = tk._attn_close(o, one, f"rank {r} vs one pass", rel_tol=F16_ATTN_TOL)
        print(f"f16 two-pass defer={defer} rank {r}: rel-L2 / tolerance {r1 / F16_ATTN_TOL:.3f} (fp32), {r2 / F16_ATTN_TOL:.3f} (one pass)")


def _two_pass(ops, Q, K, Vt, sq, skc, P, dtype, defer=8, scale=None):
    """Every rank's view of the two-pass form: local chunk first (state saved), the others in ring order, the short last block in one pass."""
    outs = []
    state = torch.zeros((Q.shape[0] * Q.shape[1], Q.shape[2], ops.STATE_LD), device=Q.device)
    for r in range(P):
        out = torch.zeros((Q.shape[0] * sq, Q.shape[1] * 128), dtype=dtype, device=Q.device)
        ops.attention(Q, K, Vt, sq, skc, out=out, nchunks=1, defer_log2=defer, rows=1, state_mode=1, state=state, chunk_first=r, chunk_total=P,
                      scale=scale)
        ops.attention(Q, K, Vt, sq, skc, out=out, nchunks=P - 1, defer_log2=defer, rows=1, state_mode=2, state=state,
                      chunk_first=(r + 1) % P, chunk_total=P, scale=scale)
        ops.attention(Q, K, Vt, sq, skc, out=out, nchunks=P, defer_log2=defer, rows=2, scale=scale)
        outs.append(out)
    return outs


@pytest.mark.parametrize("sq,skc,P,form", [(sq, skc, P, form) for (sq, skc, P) in [(300, 2100, 1), (2320, 1100, 3), (700, 16388, 4)]
                                           for form in ("one_pass", "two_pass", "forced_8wave") if P > 1 or form != "two_pass"])
def test_attention_key_coverage_f16(dev, sq, skc, P, form):
    """float16 twin of test_attention_key_coverage.  Uniform scores: p = 1, V = 1, integer sums - exact up to one rounding of count / sk
    to half (O * (1 / l)): 2^-10 relative (seen: 0.27 of it).  Tile-dependent scores: the bf16 test allows 1.5e-2 for probabilities
    rounded to bf16 (2^-9 each, systematic within a tile); half carries three more bits (2^-12 each), so 1.5e-2 / 8 = 1.875e-3
    (seen: 0.50 of it)"""
    from actionmesh_amd import ops
    for by_tile in (False, True):
        q, k, v, expect = tk._coverage_case(dev, sq, skc, P, H=1, score_by_tile=by_tile, dtype=F16)
        Q, K, Vt, skc_ = tk._layout(q, k, v, P)
        if form == "two_pass":
            outs = _two_pass(ops, Q, K, Vt, sq, skc, P, F16)
        else:
            outs = [ops.attention(Q, K, Vt, sq, skc, nchunks=P, defer_log2=98 if form == "forced_8wave" else 8)]
        for out in outs:
            o = out.double()
            assert out.dtype == F16
            if not by_tile:
                err = ((o - expect[None]).abs() / expect[None].clamp_min(1e-30)).max().item()
                print(f"f16 coverage {form} {sq}x{skc}x{P} uniform: worst error / bound {err / 2.0 ** -10:.3f}")
                assert err <= 2.0 ** -10, f"{form} uniform scores: a key tile is mis-counted (max relative error {err:.3e})"
            else:
                nz = expect > 0
                err = ((o[:, nz] - expect[None, nz]).abs() / expect[None, nz]).max().item()
                print(f"f16 coverage {form} {sq}x{skc}x{P} by tile: worst error / bound {err / 1.875e-3:.3f}")
                assert err <= 1.875e-3, f"{form} tile-dependent scores: max relative error {err:.3e}"


def test_attention_forced_rescale_branch_f16(dev):
    """float16 twin of test_attention_forced_rescale_branch: a key that dominates late forces the online-softmax rescale; re-base
    thresholds 0 and 8 must agree.  The bf16 test allows 3e-2 (two bf16 roundings at |o| up to 4); three more bits: 3.75e-3 (seen: 0.70)"""
    from actionmesh_amd import ops
    nseq, H, sq, sk = 1, 1, 256, 640
    q = _randn((nseq, H, sq, 128), 1, dev)
    k = _randn((nseq, H, sk, 128), 2, dev) * 0.3
    v = _randn((nseq, H, sk, 128), 3, dev)
    for (row, key, gain) in ((7, 333, 6.0), (100, 500, 12.0), (255, 639, 20.0), (31, 70, 9.0)):
        k[0, 0, key] = q[0, 0, row] * gain / q[0, 0, row].norm() * 11.3 / 3.0
    q, k, v = (t.half() for t in (q, k, v))
    Q, K, Vt, skc = tk._layout(q, k, v, 1)
    ref = tk._sdpa_ref(q, k, v).permute(0, 2, 1, 3).reshape(sq, 128)
    tol = 3e-2 / 8
    for base in (0, 60, 90):
        outs = []
        for defer in (base, base + 8):
            o = ops.attention(Q, K, Vt, sq, skc, defer_log2=defer).float()
            e = (o - ref).abs().max().item()
            print(f"f16 forced rescale defer={defer}: worst error / bound {e / tol:.3f}")
            assert e < tol, f"defer={defer}"
            outs.append(o)
        assert (outs[0] - outs[1]).abs().max().item() < tol


@pytest.mark.parametrize("defer", [8, 28, 98])
def test_attention_bitwise_repeatable_f16(dev, defer):
    """12 launches of the problem of test_attention_bitwise_repeatable in float16, other kernels in between: the same bits."""
    from actionmesh_amd import ops
    nseq, H, sq, sk = 2, 8, 4352, 4224
    q, k, v = _qkv(dev, nseq, H, sq, sk)
    Q, K, Vt, skc = tk._layout(q, k, v, 2)
    first = ops.attention(Q, K, Vt, sq, skc, nchunks=2, defer_log2=defer).clone()
    filler_a = _randn((4096, 1024), 4, dev).half()
    filler_w = _randn((1024, 1024), 5, dev, 0.03).half()
    for i in range(11):
        if i % 3 == 0:
            ops.gemm(filler_a, filler_w)
        out = ops.attention(Q, K, Vt, sq, skc, nchunks=2, defer_log2=defer)
        assert torch.equal(_bits(out), _bits(first)), f"launch {i + 2} differs from the first"


# ==========================================================================================================================================
# A.  elementwise kernels of the float16 build
# ==========================================================================================================================================
def test_point_embed_patchify_displacement_timestep_f16(dev):
    """The Stage II featurisation and output kernels in float16 against fp64 statements rounded once.
    point_embed: pass-through channels and the zero pad exactly; sin / cos within one half rounding (2^-11 |v|) + 1e-4 for sinf / cosf
    and the fp32 argument x * (pi 2^j) at |arg| <= 402 (ulp 3e-5) (seen: 0.71).  patchify: a gather and one rounding - exact.
    displacement: fp32 output, 4e-6 for __expf and the 2 / (1 + e) - 1 chain at |x| <= 12 (seen: 0.04).  timestep_sinusoid (the
    float16 library's kernel through the `dtype` argument): 2^-11 + 3e-4 for the fp32 argument t * expf(.) at |arg| <= 1000 (seen: 0.31)"""
    from actionmesh_amd import ops
    g = torch.Generator().manual_seed(5)
    rows, nf, ld = 1003, 8, 64
    query = (torch.rand((rows, 6), generator=g) * 2 - 1).to(dev)
    out = ops.point_embed(query, 3, 3, nf, True, ld_out=ld, dtype=F16)
    assert out.dtype == F16
    f = math.pi * 2.0 ** torch.arange(nf, device=dev, dtype=torch.float64)
    arg = (query[:, :3].double()[:, :, None] * f.float().double()[None, None]).reshape(rows, 3 * nf)
    n_used = 3 + 6 * nf + 3
    assert torch.equal(out[:, :3], query[:, :3].half()) and torch.equal(out[:, 3 + 6 * nf:n_used], query[:, 3:6].half())
    assert bool((out[:, n_used:] == 0).all())
    ref = torch.cat([arg.sin(), arg.cos()], 1)
    assert _report("f16 point_embed", (out[:, 3:3 + 6 * nf].double() - ref).abs(), 2.0 ** -11 * ref.abs() + 1e-4) <= 1.0
    # patchify: values across half's whole range (subnormal .. overflow)
    T, Cin, H, W, p = 2, 3, 28, 42, 14
    pix = (torch.randn((T, Cin, H, W), generator=g) * 10.0 ** torch.randint(-8, 6, (T, Cin, H, W), generator=g).float()).to(dev)
    ldp = ops.round_up(Cin * p * p, 64)
    out = ops.patchify(pix, p, ldp, dtype=F16)
    refp = F.unfold(pix, p, stride=p).transpose(1, 2).reshape(-1, Cin * p * p).half()
    assert torch.equal(_bits(out[:, :Cin * p * p]), _bits(refp)) and bool((out[:, Cin * p * p:] == 0).all())
    assert bool(torch.isinf(refp).any()) and bool(((refp != 0) & (refp.abs() < 2.0 ** -14)).any())
    # displacement
    logits = (torch.randn((777, 8), generator=g) * 4).half().to(dev)
    o = ops.displacement(logits, 3, torch.empty((777, 3), device=dev))
    refd = 2.0 * torch.sigmoid(-logits[:, :3].double()) - 1.0
    assert _report("f16 displacement", (o.double() - refd).abs(), torch.full_like(refd, 4e-6)) <= 1.0
    # timestep_sinusoid
    t = torch.tensor([1000.0, 0.0, 8.9285717, 523.25, 964.40027], device=dev)
    o = ops.timestep_sinusoid(t, 256, dtype=F16)
    assert o.dtype == F16
    fr = torch.exp(-math.log(10000.0) * torch.arange(128, dtype=torch.float64, device=dev) / 128)
    reft = torch.cat([torch.sin(t.double()[:, None] * fr), torch.cos(t.double()[:, None] * fr)], -1)
    assert _report("f16 timestep_sinusoid", (o.double() - reft).abs(), torch.full_like(reft, 2.0 ** -11 + 3e-4)) <= 1.0
    assert torch.equal(ops.timestep_sinusoid(t, 256), ops.timestep_sinusoid(t, 256, dtype=BF16))       # the default is the bf16 library


# ==========================================================================================================================================
# B.  exact arithmetic
# ==========================================================================================================================================
def _ints(shape, seed, dev, lo=-15, hi=15):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).double().to(dev)


def _exact_routes(M):
    return ["dispatch"] if M > 30000 else list(ROUTES)


EXACT_SHAPES = [(300, 264), (2048 + 256 + 40, 264), (33792 + 32, 1024)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(M, N, K) for (M, N) in EXACT_SHAPES for K in (64, 4096) if M < 30000 or K == 64])
def test_gemm_exact_subnormal_operands(dev, dtype, M, N, K):
    """A = integers in [-15, 15] x 2^-24 (in half: zero or SUBNORMAL, every entry), W = integers in [-15, 15] x 2^8.  Both are exact in
    half and bf16; products are integers x 2^-16 and any partial sum stays below 15 x 15 x 4096 < 2^24 units: fp32 accumulation is exact
    in ANY order, so the output must EQUAL the fp64 product rounded once - bit for bit, every element, every kernel (2344 rows under
    force_big = 9 tiles of 256 + 40 rows in gemm_tail_kernel; 33 824 x 1024: the product dispatch's big path + tail kernel; K = 64 there
    only, to keep the reference small).  An MFMA that flushed subnormal operands would return all zeros; a dropped or doubled k-slice
    cannot hide under a tolerance."""
    from actionmesh_amd import ops
    a = (_ints((M, K), 1, dev) * 2.0 ** -24).to(dtype)
    w = (_ints((N, K), 2, dev) * 2.0 ** 8).to(dtype)
    assert torch.equal(a.double(), _ints((M, K), 1, dev) * 2.0 ** -24)                    # the operands are exact in the type
    if dtype == F16:
        assert bool((a.abs().float() < 2.0 ** -14).all())
    ref = (a.double() @ w.double().T)
    want = ref.float().to(dtype)
    assert bool((want != 0).any())
    for r in _exact_routes(M):
        out = ops.gemm(a, w, **ROUTES[r])
        bad = _bits(out) != _bits(want)
        print(f"{dtype} exact gemm {M}x{N}x{K} {r}: {int(bad.sum())} of {bad.numel()} elements differ")
        assert not bool(bad.any()), f"{r}: {int(bad.sum())} elements differ, first at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("K", [64, 4096])
@pytest.mark.parametrize("M,N", EXACT_SHAPES[:2])
def test_gemm_exact_subnormal_outputs_f16(dev, M, N, K):
    """The same with W scaled by a further 2^-12 (integers x 2^-4): products are integers x 2^-28, the sums exact in fp32, and almost
    every non-zero output lies in half's subnormal range and needs rounding to a multiple of 2^-24 (ties included): bitwise against
    fp64 -> fp32 (exact) -> half."""
    from actionmesh_amd import ops
    a = (_ints((M, K), 3, dev) * 2.0 ** -24).half()
    w = (_ints((N, K), 4, dev) * 2.0 ** -4).half()
    ref = a.double() @ w.double().T
    want = ref.float().half()
    nzero = ref != 0
    sub = nzero & (ref.abs() < 2.0 ** -14)
    inexact = nzero & (want.double() != ref)
    tie = nzero & ((ref * 2.0 ** 25) % 2 == 1)
    print(f"f16 subnormal outputs {M}x{N}x{K}: {float(sub.sum()) / float(nzero.sum()):.3f} of the non-zero outputs subnormal, "
          f"{float(inexact.sum()) / float(nzero.sum()):.3f} rounded, {int(tie.sum())} ties")
    assert float(sub.sum()) > 0.5 * float(nzero.sum()) and int(tie.sum()) > 0
    for r in ROUTES:
        out = ops.gemm(a, w, **ROUTES[r])
        bad = _bits(out) != _bits(want)
        print(f"    {r}: {int(bad.sum())} of {bad.numel()} elements differ")
        assert not bool(bad.any()), f"{r}: {int(bad.sum())} elements differ, first at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("mode", ["plain", "bias", "bias_res", "bias_gelu"])
@pytest.mark.parametrize("M,N", EXACT_SHAPES[:2])
def test_gemm_exact_overflow_f16(dev, M, N, mode):
    """A = integers in [-15, 15], W = integers x 32, K = 256: sums are integers up to 15 x 480 x 256 < 2^24 (fp32-exact) and about a
    tenth of them leave half's range.  IEEE rounding: |x| < 65520 -> at most 65504, |x| >= 65520 -> a SIGNED infinity - not a saturated,
    wrapped or NaN value.  Planted: row 0 hits +65504 in column 0; with a bias columns 1 and 2 repeat column 0 with bias 15 (65519 ->
    65504) and 16 (65520 -> +inf); row 1 is row 0 negated.  bias_res follows the kernel's rounding points (round the linear, add the
    residual in fp32, round): the residual turns a 65504 into 65520 -> inf in one planted element.  All bitwise.  GELU: finite exactly
    where F.gelu of the rounded linear is, and there within the GEMM bound of part A (torch's own gelu(+inf) is NaN, so the sign of a
    non-finite result is not asserted)."""
    from actionmesh_amd import ops
    K = 256
    a = _ints((M, K), 5, dev)
    w = _ints((N, K), 6, dev) * 32.0
    a[0] = 0; a[0, :9] = 15; a[0, 9] = 11
    a[1] = -a[0]
    w[0] = 0; w[0, :9] = 480; w[0, 9] = 64                     # 9 x 15 x 480 + 11 x 64 = 65504
    w[1] = w[0]; w[2] = w[0]
    bias = res = None
    if mode != "plain":
        bias = _ints((N,), 7, dev).float()
        bias[0], bias[1], bias[2] = 0.0, 15.0, 16.0
    if mode == "bias_res":
        res = (_randn((M, N), 8, dev) * 2.0e4).clamp(-6.0e4, 6.0e4).half()          # finite: inf - inf would be a NaN of the test's own making
        res[0, 0] = 16.0                                       # 65504 + 16 = 65520 -> inf
        res[1, 0] = 16.0                                       # -65504 + 16: finite
        res[0, 1] = -32.0                                      # 65504 (from 65519) - 32 = 65472: exact
    a, w = a.half(), w.half()
    ref, lin = _gemm_ref(a, w, bias, res, mode == "bias_gelu")
    assert float(lin[0, 0]) == 65504.0 and float(lin[1, 0]) == -65504.0
    if mode != "plain":
        assert float(lin[0, 1]) == 65504.0 and float(lin[0, 2]) == float("inf")          # 65519 -> 65504, 65520 -> +inf
        assert float(lin[1, 1]) == -65504.0 and float(lin[1, 2]) == -65472.0             # -65489 -> -65504; -65488 is a tie -> even
    if mode == "bias_res":
        assert float(ref[0, 0]) == float("inf") and math.isfinite(float(ref[1, 0])) and float(ref[0, 1]) == 65472.0
    frac = float(torch.isinf(lin).float().mean())
    print(f"f16 overflow {M}x{N} {mode}: {frac:.3f} of the linears infinite, max |sum| {float((a.double() @ w.double().T).abs().max()):.0f}")
    assert frac > 0.03 and not bool(torch.isnan(lin).any())
    want = ref.float().half()
    for r in ROUTES:
        out = ops.gemm(a, w, bias=bias, residual=res, gelu=(mode == "bias_gelu"), **ROUTES[r])
        if mode == "bias_gelu":
            fin = torch.isfinite(ref)
            assert torch.equal(torch.isfinite(out), fin), f"{r}: GELU finite where the reference is not (or the reverse)"
            err = torch.where(fin, (out.double() - ref).abs(), torch.zeros_like(ref))
            rr, ll = torch.where(fin, ref, torch.zeros_like(ref)), torch.where(fin, lin, torch.zeros_like(lin))
            assert _report(f"    {r} gelu on the finite part", err, _gemm_bound(rr, ll)) <= 1.0
        else:
            assert not bool(torch.isnan(out).any()), f"{r}: NaN"
            bad = _bits(out) != _bits(want)
            print(f"    {r}: {int(bad.sum())} of {bad.numel()} elements differ")
            assert not bool(bad.any()), f"{r}: {int(bad.sum())} elements differ, first at {bad.nonzero()[0].tolist()}"


def _specials(dtype):
    """fp32 values at the edges of the 16-bit type: [largest finite, the last value that rounds to it, the first that rounds to inf,
    smallest subnormal s, s / 2 (tie -> 0), just above s / 2 (-> s), 1.5 s (tie -> 2 s), the normal / subnormal boundary tie, ties at 1]."""
    if dtype == F16:
        big, nxt, s, mn, e = 65504.0, 65520.0, 2.0 ** -24, 2.0 ** -14, 2.0 ** -11
    else:
        big, nxt, s, mn, e = 2.0 ** 127 * (2 - 2.0 ** -7), 2.0 ** 127 * (2 - 2.0 ** -8), 2.0 ** -133, 2.0 ** -126, 2.0 ** -8
    x = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), big, -big, nxt, -nxt, s, -s, s / 2, -s / 2, 1.5 * s, 2.5 * s,
                      mn - s / 2, mn + s / 2, -(mn - s / 2), 1 + e, 1 + 3 * e, -(1 + e), 1 + e + 2.0 ** -23, 1 + e - 2.0 ** -23],
                     dtype=torch.float64).float()
    below = torch.nextafter(torch.tensor([nxt, -nxt, s / 2, -s / 2]), torch.tensor([0.0, 0.0, 1.0, -1.0]))
    return torch.cat([x, below])


@pytest.mark.parametrize("dtype", DTYPES)
def test_f32_to_16_exact_at_the_edges(dev, dtype):
    """am_f32_to_bf16 of both builds against torch's CPU conversion, bit for bit (NaNs by isnan): +-0, +-inf, NaN, the largest finite value,
    the last value below the overflow threshold and the threshold itself, the smallest subnormal, half of it (tie -> 0) and the next
    float above (-> subnormal), ties at subnormal / normal values, and 10^6 random magnitudes 2^-30 .. 2^17 (for half: from under the
    smallest subnormal to over the largest finite value).  The length is not a multiple of 8 and the specials sit at BOTH ends, so the
    vector path (hardware convert, pack_bf2) and the scalar tail (f2bf) both see them."""
    from actionmesh_amd import ops
    g = torch.Generator().manual_seed(9)
    n = 1000003
    mag = torch.exp2(torch.rand(n, generator=g, dtype=torch.float64) * 47.0 - 30.0)
    body = (mag * (torch.randint(0, 2, (n,), generator=g).double() * 2 - 1)).float()
    sp = _specials(dtype)
    x = torch.cat([sp, body, sp.flip(0)[:5], sp])
    if x.numel() % 8 == 0:
        x = torch.cat([x, sp[:3]])
    assert x.numel() % 8 != 0
    want = x.to(dtype)
    got = ops.f32_to_bf16(x.to(dev), dtype=dtype).cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    bad = (_bits(got) != _bits(want)) & ~nan
    print(f"{dtype} f32 -> 16: {int(bad.sum())} of {x.numel()} differ; {int(torch.isinf(want).sum())} inf, "
          f"{int(((want != 0) & (want.float().abs() < float(torch.finfo(dtype).tiny))).sum())} subnormal, {int((want == 0).sum())} zero")
    assert not bool(bad.any()), f"first at {bad.nonzero()[0].tolist()}: x = {float(x[bad.nonzero()[0][0]])!r}"


# ==========================================================================================================================================
# C.  softmax probabilities in half's subnormal range
# ==========================================================================================================================================
LN2 = math.log(2.0)


def _peaky_case(dev, dtype, sq, skc, P, G, where):
    """tk._coverage_case with ONE dominant key: Q = e0, every tail key K = 0 (score exactly 0), the dominant key K = G e0, and
    scale = ln 2, so that scores are the integers 0 and G in the kernels' log2 units and every probability is an exact power of two.
    V = tile indicator on the tail keys, 1 + c / 128 in channel c on the dominant key.  Expected (fp64, the same for every row):
    (v_dom + 2^-G count_c) / (1 + n_tail 2^-G), count_c from the TRUE key count: the zero keys that pad a chunk's last tile must not
    count (they are masked to -inf by the kernels)."""
    n = skc * P
    tiles_c = (skc + 63) // 64
    key = torch.arange(skc, device=dev)
    gt = torch.cat([c * tiles_c + key // 64 for c in range(P)])
    dom = {"first": 0, "last": n - 1, "middle": (2 * skc + skc // 2) if P >= 3 else n // 2}[where]
    q = torch.zeros((1, 1, sq, 128), device=dev); q[..., 0] = 1.0
    k = torch.zeros((1, 1, n, 128), device=dev); k[0, 0, dom, 0] = float(G)
    v = torch.zeros((1, 1, n, 128), device=dev)
    v[0, 0, torch.arange(n, device=dev), gt % 128] = 1.0
    vd = 1.0 + torch.arange(128, device=dev, dtype=torch.float64) / 128
    v[0, 0, dom] = vd.float()
    count = torch.zeros(128, dtype=torch.float64, device=dev).index_add_(0, gt % 128, torch.ones(n, dtype=torch.float64, device=dev))
    count[gt[dom] % 128] -= 1
    expect = (vd + 2.0 ** -G * count) / (1.0 + (n - 1) * 2.0 ** -G)
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    assert float(k[0, 0, dom, 0]) == G and torch.equal(v[0, 0, dom].double(), vd)
    # the kernels form c = scale * log2(e) in fp32 and re-round Q * c to the 16-bit type: that must return Q itself
    c = torch.tensor(LN2, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    assert torch.equal((q.float() * c.to(dev)).to(dtype), q)
    return q, k, v, expect, (n - 1) * 2.0 ** -G / (1.0 + (n - 1) * 2.0 ** -G)


PEAKY = [(4224, 1, 12), (16388, 4, 16), (16388, 4, 20), (16388, 4, 24)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", ["first", "last", "middle"])
@pytest.mark.parametrize("skc,P,G", PEAKY)
def test_attention_subnormal_probabilities(dev, dtype, skc, P, G, where):
    """In float16 P = exp2(s - m) is subnormal as soon as a key sits more than 14 octaves under the row maximum.  65 551 keys 16 octaves
    under one dominant key carry HALF of the softmax mass (65 551 x 2^-16 = 1.0002); at 24 octaves 0.39 %, four times the tolerance.  If
    one of the three consumers of P - the 16-bit convert, the P.V MFMA, the row sum (v_dot2c_f32_f16 in the 4x64 kernel) - flushed
    subnormals, or the numerator (MFMA) and the denominator disagreed, the output would be off by that share.  For G <= 24 every P is an
    exact power of two representable in half whatever the deferred re-base lag, so the only rounding is the output's: 2^-10 relative
    (bf16: 2^-7, as in test_attention_key_coverage; it has the range and pins the construction).  4224 keys x 12 octaves is the
    normal-range control.  The dominant key sits in tile 0 (the tail is exponentiated against the final maximum from the start), in the
    last tile (O is rescaled by 2^-G at the very end) or in the middle of chunk 2.  Forms: product dispatch, forced 8-wave (90 / 98),
    forced 4x64 (60 / 68), and the two-pass form (2320 query rows: 9 full blocks + a short one; the dominant key is in the local chunk
    of one rank and in a remote chunk of the others).  With V = 1 on every key the output must be 1: numerator and denominator treat the
    same P alike.  seen: worst error / bound 0.48 (f16), 0.50 (bf16)"""
    from actionmesh_amd import ops
    tol = 2.0 ** -10 if dtype == F16 else 2.0 ** -7
    worst = {}
    for sq, forms in ((300, (8, 90, 98, 60, 68)), (2320, ("two_pass",) if P > 1 else ())):
        if not forms:
            continue
        q, k, v, expect, share = _peaky_case(dev, dtype, sq, skc, P, G, where)
        Q, K, Vt, skc_ = tk._layout(q, k, v, P)
        ones = torch.ones_like(Vt)
        for form in forms:
            if form == "two_pass":
                outs = _two_pass(ops, Q, K, Vt, sq, skc, P, dtype, defer=8, scale=LN2)
                outs1 = _two_pass(ops, Q, K, ones, sq, skc, P, dtype, defer=8, scale=LN2)
            else:
                outs = [ops.attention(Q, K, Vt, sq, skc, nchunks=P, defer_log2=form, scale=LN2)]
                outs1 = [ops.attention(Q, K, ones, sq, skc, nchunks=P, defer_log2=form, scale=LN2)]
            for i, (o, o1) in enumerate(zip(outs, outs1)):
                e = float(((o.double() - expect[None]).abs() / expect[None]).max())
                e1 = float((o1.double() - 1.0).abs().max())
                worst[(form, i)] = max(e, e1) / tol
                assert e <= tol, f"{form} rank {i}: max relative error {e:.3e} (the tail carries {share:.3%} of the mass)"
                assert e1 <= tol, f"{form} rank {i}: V = 1 gives {e1:.3e} off 1"
    print(f"{dtype} peaky softmax {skc}x{P} G={G} {where} (tail share {share:.3%}): worst error / bound "
          + ", ".join(f"{f}{'/' + str(i) if f == 'two_pass' else ''} {w:.2f}" for (f, i), w in worst.items()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", ["first", "last"])
def test_attention_probabilities_below_half(dev, dtype, where):
    """G = 26: P = 2^-26 is below half's smallest subnormal (2^-24) and below the tie to it (2^-25), so the P.V MFMA of the float16 build
    cannot see these keys (a kernel that sums its rows in fp32 still counts them in the denominator).  That is the float16 build's
    STATED LIMIT - the values of keys more than 24 octaves under the row maximum do not count - and the assertion is only that the
    deviation from fp64 is at most the tail's own share of the mass (9.8e-4 at 65 552 keys) plus the output rounding.  bf16 has the
    range: its legs stay within the output rounding alone.  seen: f16 0.17 of the bound on all three forms (3.2e-4, i.e. the rounding
    of the output: the tail's values carry 5e-6 here, its mass is kept by the fp32 row sums), bf16 0.13."""
    from actionmesh_amd import ops
    skc, P, G, sq = 16388, 4, 26, 300
    q, k, v, expect, share = _peaky_case(dev, dtype, sq, skc, P, G, where)
    Q, K, Vt, skc_ = tk._layout(q, k, v, P)
    tol = (share + 2.0 ** -10) if dtype == F16 else 2.0 ** -7
    for form in (8, 90, 60):
        o = ops.attention(Q, K, Vt, sq, skc, nchunks=P, defer_log2=form, scale=LN2)
        e = float(((o.double() - expect[None]).abs() / expect[None]).max())
        print(f"{dtype} G=26 {where} defer={form} (tail share {share:.2e}): worst error / bound {e / tol:.3f}")
        assert e <= tol, (form, e)


# ==========================================================================================================================================
# C.  norms and elementwise kernels at the edges of half's range
# ==========================================================================================================================================
def test_layernorm_and_rmsnorm_on_subnormal_and_huge_rows_f16(dev):
    """Rows whose every entry is a half subnormal: the variance (<= 2^-28) is far below eps, so LayerNorm gives (x - mean) rsqrt(var + eps) w + b
    ~ x * 316 w + b and head_post's RMSNorm x * rsqrt(eps) w = x * 1000 w - inputs read as zero would give b / 0.  Rows near +-60 000:
    squares of 3.6e9 and sums of 3.7e12 are ordinary fp32, the output is +-1 w + b.  Against fp64; tolerance of the twins (1.5
    roundings of 2^-11) with the absolute term replaced by one subnormal spacing, 2^-24, on the subnormal rows (outputs there are
    <= 0.03, where the twins' 1e-5 would hide a flush of the smaller inputs) (seen: LayerNorm 0.66 / 0.66, RMSNorm 0.65 / 0.66)"""
    from actionmesh_amd import ops
    C, rows = 1024, 64
    g = torch.Generator().manual_seed(21)
    sub = (torch.randint(-63, 64, (rows, C), generator=g).double() * 2.0 ** -24).to(dev).half()
    assert bool((sub.float().abs() < 2.0 ** -14).all()) and bool((sub != 0).any())
    huge = ((torch.randint(0, 2, (rows, C), generator=g).double() * 2 - 1) * (60000.0 + 32.0 * torch.randint(-50, 50, (rows, C), generator=g))).to(dev).half()
    assert bool(torch.isfinite(huge).all()) and float(huge.float().abs().min()) > 58000
    w = _randn((C,), 2, dev) * 0.2 + 1.0
    b = _randn((C,), 3, dev) * 0.2
    for name, x, atol in (("subnormal", sub, 2.0 ** -24), ("huge", huge, 1e-5)):
        out = ops.layernorm(x, w, b, 1e-5)
        ref = F.layer_norm(x.double(), (C,), w.double(), b.double(), 1e-5)
        _close(out, ref, 1.5, atol, f"f16 layernorm on {name} rows")
        if name == "subnormal":                               # the signal itself, not just b: (out - b) / w must follow x
            sig = ((out.double() - b.double()) / w.double()).abs().mean() / (sub.double().abs().mean() * 1e-5 ** -0.5)
            print(f"    signal / expected {float(sig):.3f}")
            assert 0.9 < float(sig) < 1.1
    heads, L = 2, 64
    wq = _randn((128,), 4, dev) * 0.2 + 1.0
    for name, x, atol in (("subnormal", sub[:, :heads * 128].contiguous(), 2.0 ** -24), ("huge", huge[:, :heads * 128].contiguous(), 1e-5)):
        qo, _, _ = ops.head_post(x, heads, (0,), L, L, w_q=wq)
        xs = x.double().view(rows, heads, 128)
        ref = (xs * torch.rsqrt(xs.pow(2).mean(-1, keepdim=True) + 1e-6) * wq.double()).view(rows // L, L, heads, 128).permute(0, 2, 1, 3)
        _close(qo[:, :, :L], ref, 1.5, atol, f"f16 head_post RMSNorm on {name} rows")
        if name == "subnormal":
            assert float(ref.abs().max()) > 1e-3


def test_displacement_and_flow_step_at_the_edges_f16(dev):
    """displacement on +-65504 and +-inf logits: 2 sigmoid(-x) - 1 = -+1 exactly (no NaN from inf arithmetic).  flow_step where
    dt * v lands in half's subnormal range: the update is rounded to a multiple of 2^-24 and must not vanish - bit for bit the half
    arithmetic of test_layernorm_and_flow_step_f16 (CFG rounded at every op, dt * v rounded, fp32 add) on latents of 0 and of 1e-3."""
    from actionmesh_amd import ops
    inf = float("inf")
    logits = torch.tensor([[65504.0, -65504.0, inf, -inf, 0.0, -0.0, 20.0, -20.0]], device=dev).half()
    o = ops.displacement(logits, 8, torch.empty((1, 8), device=dev)).cpu()
    assert torch.equal(o[0, :6], torch.tensor([-1.0, 1.0, -1.0, 1.0, 0.0, 0.0])), o
    assert abs(float(o[0, 6]) + 1) < 1e-6 and abs(float(o[0, 7]) - 1) < 1e-6
    g = torch.Generator().manual_seed(4)
    T, N, D = 3, 17, 64
    v = (torch.randn(2, T, N, D, generator=g) * 1e-4).half()
    dt = torch.tensor(0.0371, dtype=torch.float32)
    d = (v[1].float() - v[0].float()).half()
    vv = (v[0].float() + (7.5 * d.float()).half().float()).half()
    upd = (dt * vv.float()).half().float()
    sub = (upd != 0) & (upd.abs() < 2.0 ** -14)
    print(f"f16 flow_step: {float(sub.float().mean()):.3f} of the updates subnormal, {float((upd == 0).float().mean()):.3f} zero")
    assert float(sub.float().mean()) > 0.7
    for base in (0.0, 1e-3):
        lat = torch.full((T, N, D), base)
        want = lat.clone()
        want[1:] = lat[1:] + upd[1:]
        got = lat.clone().to(dev)
        ops.flow_step(v.to(dev), got, [7.5], 0.0371, True, [False, True, True])
        assert torch.equal(got.cpu(), want), f"base {base}: {int((got.cpu() != want).sum())} elements differ"
    assert bool((want[1:] != 1e-3).float().mean() > 0.7)        # the subnormal updates moved the fp32 latents
