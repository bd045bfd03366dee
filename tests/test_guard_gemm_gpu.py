"""Guard bands and leading dimensions of am_gemm_bf16 (both library builds): every GEMM route writes C[r][0 .. N) of its M rows and
nothing else, reads nothing outside its operands, and gives the same bits whatever the leading dimensions.

Every operand and every output lives in an arena (tests/_guard.py): 256 sentinel rows in front and behind, and - layout L1 - padded
rows (lda = K + 8, ldw = K + 24, ldc = N + 8, lda2 = K2 + 16) whose gap columns hold the sentinel too.  The sentinel is a NaN: a read
outside an operand poisons the result, a store outside the output changes a sentinel.  Each case asserts
  (a) all guards and gaps of every arena are untouched,
  (b) the values against the fp64 statement of test_f16_kernels_gpu.py (`_gemm_ref`), at the bound the route's own test uses,
  (c) the same bits as the same call on exactly-sized contiguous tensors.
Every test prints its worst error / bound."""
import math

import pytest
import torch
import torch.nn.functional as F

import test_f16_kernels_gpu as tf
import test_kernels_gpu as tk
from _guard import SENTINEL, Arena

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = tf.DTYPES
ROUTES = tf.ROUTES
EPS16 = {F16: 2.0 ** -11, BF16: 2.0 ** -8}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from actionmesh_amd import _lib
    _lib.lib()
    _lib.lib("f16")
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int16)


def _check_values(out, ref, lin, res, K, gelu, route, dtype, what):
    """float16: `_gemm_bound` (test_gemm_routes_f16).  bfloat16: `_close` with the parameters of test_gemm / test_gemm256_pingpong_main_loop
    (2 relative ulp - 4 in the GELU mode of the 256x256 tile - of max(|value|, |linear|, |residual|) + 2e-3 sqrt(K / 64))."""
    if dtype == F16:
        worst = tf._report(what, (out.double() - ref).abs(), tf._gemm_bound(ref, lin))
        assert worst <= 1.0, f"{what}: worst error / bound {worst:.3f}"
        return worst
    mag = lin.abs() if res is None else torch.maximum(lin.abs(), res.double().abs())
    ulps = 4.0 if (gelu and route in ("big", "lockstep")) else 2.0
    return tf._close(out, ref, ulps, 2e-3 * math.sqrt(K / 64), what, mag=mag, dtype=BF16)


# (M, N, K, route): what the shape reaches is in the docstring of test_gemm_guards_and_leading_dimensions
CASES = [(1, 8, 64, "small"), (37, 72, 128, "small"), (129, 136, 64, "small"),
         (300, 328, 192, "big"), (300, 328, 192, "lockstep"), (513, 264, 64, "big"), (513, 264, 64, "lockstep"),
         (2088, 72, 128, "big")]
MODES = ["plain", "bias_gelu", "bias_res", "bias_res_alias", "split"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,N,K,route", CASES)
def test_gemm_guards_and_leading_dimensions(dev, M, N, K, route, mode, dtype):
    """(1, 8, 64): minimal M and N; (37, 72, 128), (129, 136, 64): M and N tails of the 128x128 tile; (300, 328, 192): one partial
    256x256 tile in both directions; (513, 264, 64): partial 256 tiles behind full ones in both directions; (2088, 72, 128) under
    force_big: M > 2048 with remainder 40, so gemm_tail_kernel gets 32 + 8 rows and its second 64-column block holds 8 valid columns.
    Layouts L0 (natural, guard rows only) and L1 (every leading dimension padded); the residual in its own arena with C's leading
    dimension, or aliasing C.  Split A needs two K blocks of 64: K = 64 shapes run it with K doubled.
    seen (worst error / bound over all cases): bf16 0.44, f16 0.40"""
    from actionmesh_amd import ops
    if mode == "split" and K == 64:
        K = 128
    a = tk._randn((M, K), 1, dev).to(dtype)
    w = tk._randn((N, K), 2, dev, 1.0 / math.sqrt(K)).to(dtype)
    bias = tk._randn((N,), 3, dev, 0.5) if mode.startswith("bias") else None
    res = tk._randn((M, N), 4, dev).to(dtype) if "res" in mode else None
    gelu = mode == "bias_gelu"
    K1 = 64 if mode == "split" else K
    kw = dict(bias=bias, gelu=gelu, **ROUTES[route])
    ref, lin = tf._gemm_ref(a, w, bias, res, gelu)

    def call(A1, A2, W, R, C):
        return ops.gemm(A1, W, a2=A2, residual=R, out=C, **kw)

    # the same call on exactly-sized contiguous tensors
    a1c, a2c = (a[:, :K1].contiguous(), a[:, K1:].contiguous()) if mode == "split" else (a, None)
    if mode == "bias_res_alias":
        base = res.clone()
        call(a1c, a2c, w, base, base)
    else:
        base = call(a1c, a2c, w, res, None)
    for layout in ("L0", "L1"):
        pad = (lambda n: n) if layout == "L1" else (lambda n: 0)
        A1 = Arena.of(a1c, ld=K1 + pad(8))
        A2 = Arena.of(a2c, ld=(K - K1) + pad(16)) if a2c is not None else None
        W = Arena.of(w, ld=K + pad(24))
        C = Arena(M, N, dtype, dev, ld=N + pad(8))
        R = None
        if mode == "bias_res":
            R = Arena.of(res, ld=N + pad(8))
        elif mode == "bias_res_alias":
            C.view.copy_(res)
        call(A1.view, A2.view if A2 else None, W.view, C.view if mode == "bias_res_alias" else (R.view if R else None), C.view)
        torch.cuda.synchronize()
        what = f"{dtype} gemm {M}x{N}x{K} {route} {mode} {layout}"
        for nm, ar in (("C", C), ("A1", A1), ("A2", A2), ("W", W), ("residual", R)):
            if ar is not None:
                ar.assert_untouched(f"{what}: {nm}")
        _check_values(C.view, ref, lin, res, K, gelu, route, dtype, what)
        bad = _bits(C.view) != _bits(base)
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ from the contiguous call, first at {bad.nonzero()[0].tolist()}"
        if R is not None:
            assert torch.equal(_bits(R.view), _bits(res)), f"{what}: the residual operand was modified"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K,route", [(37, 72, 128, "small"), (300, 328, 192, "big"), (513, 256, 64, "big"), (2088, 72, 128, "big"),
                                         (2304 + 40, 512, 64, "big")])
def test_gemm_folded_layernorm_and_row_parts_guards(dev, M, N, K, route, dtype):
    """The folded-LayerNorm consumer that is also a statistics producer: gemm(x, W', bias=d, ln=(stats, colsum), ln_part=part) with
    x, W', C padded (L1) and `part` (M, ceil(N / 256), 2) in a guarded fp32 arena.  N % 256 == 0 at (513, 256, 64) and (2344, 512, 64):
    the full 256-row tiles of the ping-pong kernel write their slices from the store loop (512 / 2304 rows), the rest - and every row of the
    other shapes - comes from the read-back pass over C, which has to honour ldc.  Values: test_ln_fold_gpu.py's bounds - rel-L2 of the
    folded linear against the fp64 LayerNorm + linear < 0.75 x the type's rounding unit; every slice's (mean, M2) against the fp64
    statistics of the stored C at rtol 1e-5 / 2e-5, atol 1e-5.
    seen: folded rel-L2 / bound bf16 0.69, f16 0.69; parts 0.01 of their tolerance"""
    from actionmesh_amd import ops
    x = (tk._randn((M, K), 4, dev) * 1.7 + 0.4).to(dtype)
    w = tk._randn((N, K), 5, dev, K ** -0.5).to(dtype)
    gamma = tk._randn((K,), 6, dev).abs() * 0.5 + 0.5
    beta = tk._randn((K,), 7, dev) * 0.2
    bias = tk._randn((N,), 8, dev).to(dtype).float()
    wf, colsum, d = ops.ln_fold_weight(w, gamma, beta, bias)
    st = ops.row_stats(x)
    nparts = (N + 255) // 256
    kw = dict(bias=d, ln=(st, colsum), **ROUTES[route])
    part0 = torch.empty((M, nparts, 2), dtype=torch.float32, device=dev)
    base = ops.gemm(x, wf, ln_part=part0, **kw)
    ref = F.layer_norm(x.double(), (K,), gamma.double(), beta.double(), 1e-5) @ w.double().T + bias.double()
    for layout in ("L0", "L1"):
        pad = (lambda n: n) if layout == "L1" else (lambda n: 0)
        X, W = Arena.of(x, ld=K + pad(8)), Arena.of(wf, ld=K + pad(24))
        C = Arena(M, N, dtype, dev, ld=N + pad(8))
        P = Arena.flat((M, nparts, 2), torch.float32, dev)
        ops.gemm(X.view, W.view, out=C.view, ln_part=P.view, **kw)
        torch.cuda.synchronize()
        what = f"{dtype} folded gemm {M}x{N}x{K} {route} {layout}"
        for nm, ar in (("C", C), ("x", X), ("W'", W), ("ln_part", P)):
            ar.assert_untouched(f"{what}: {nm}")
        e = tf._rel(C.view, ref) / (0.75 * EPS16[dtype])
        print(f"{what}: rel-L2 / bound {e:.3f}")
        assert e < 1.0
        assert torch.equal(_bits(C.view), _bits(base)), f"{what}: differs from the contiguous call"
        assert torch.equal(P.view.view(torch.int32), part0.view(torch.int32)), f"{what}: ln_part differs from the contiguous call"
        o = C.view.double()
        worst = 0.0
        for j in range(nparts):
            sl = o[:, j * 256:(j + 1) * 256]
            mean = sl.mean(-1)
            m2 = ((sl - mean[:, None]) ** 2).sum(-1)
            worst = max(worst, float(((P.view[:, j, 0].double() - mean).abs() / (1e-5 + 1e-5 * mean.abs())).max()),
                        float(((P.view[:, j, 1].double() - m2).abs() / (1e-5 + 2e-5 * m2.abs())).max()))
        print(f"{what}: ln_part worst error / tolerance {worst:.3f}")
        assert worst <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_row_map_behind_the_grid_leaves_every_unmapped_row(dev, dtype):
    """The 43-frame row-map shape of test_gemm256_row_maps_with_a_remainder_behind_the_grid (2064 rows = 8 x 256 + 16 under force_big:
    launch_tail hands the 16 remainder rows, with their row maps, to the 128x128 tile at m_base = 2048), split A, in-place residual,
    N = 328.  C starts as sentinels everywhere; the residual values are written into the mapped rows (1 .. 48 of every 49-row frame)
    only, so row 0 of EVERY frame, the gap columns of L1 and the guard rows must all come back as sentinels.
    float16: the GEMM bound; bf16: the bound of the 30-frame twin (2 ulp + 4e-3).  seen: f16 0.59, bf16 0.49"""
    from actionmesh_amd import ops
    frames, G, L, N, K1, K2 = 43, 48, 49, 328, 128, 64
    M = frames * G
    a1 = tk._randn((frames * L, K1), 1, dev).to(dtype)
    a2 = tk._randn((frames * L, K2), 2, dev).to(dtype)
    w = tk._randn((N, K1 + K2), 3, dev, 0.07).to(dtype)
    bias = tk._randn((N,), 4, dev, 0.5).to(dtype).float()
    res = tk._randn((frames, G, N), 5, dev).to(dtype)
    cat = torch.cat([a1, a2], 1).view(frames, L, K1 + K2)[:, 1:].reshape(M, K1 + K2)
    ref, lin = tf._gemm_ref(cat, w, bias, res.reshape(M, N), False)
    outs = []
    for layout in ("L0", "L1"):
        pad = (lambda n: n) if layout == "L1" else (lambda n: 0)
        A1, A2, W = Arena.of(a1, ld=K1 + pad(8)), Arena.of(a2, ld=K2 + pad(16)), Arena.of(w, ld=K1 + K2 + pad(24))
        C = Arena(frames * L, N, dtype, dev, ld=N + pad(8))
        torch.as_strided(C.raw, (frames, G, N), (L * C.ld, C.ld, 1), C.origin + C.ld).copy_(res)
        ops.gemm(A1.view, W.view, bias=bias, a2=A2.view, residual=C.view, out=C.view, a_map=(G, L, 1), c_map=(G, L, 1), M=M, force_big=True)
        torch.cuda.synchronize()
        what = f"{dtype} row-mapped gemm {layout}"
        for nm, ar in (("C", C), ("A1", A1), ("A2", A2), ("W", W)):
            ar.assert_untouched(f"{what}: {nm}")
        got = C.view.view(frames, L, N) if layout == "L0" else torch.as_strided(C.raw, (frames, L, N), (L * C.ld, C.ld, 1), C.origin)
        row0 = _bits(got[:, 0])
        assert bool((row0 == SENTINEL[dtype]).all()), f"{what}: row 0 of {int((row0 != SENTINEL[dtype]).any(-1).sum())} frames was written"
        o = got[:, 1:].reshape(M, N)
        if dtype == F16:
            assert tf._report(what, (o.double() - ref).abs(), tf._gemm_bound(ref, lin)) <= 1.0
        else:
            r2 = res.reshape(M, N).double()
            tf._close(o, lin + r2, 2.0, 4e-3, what, mag=torch.maximum(lin.abs(), r2.abs()), dtype=BF16)
        outs.append(o.contiguous())
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "natural and padded layouts differ"


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_bias_alignment(dev, dtype):
    """The bias is fp32 and any float pointer is a valid bias for the 128x128 tile, which reads it one float at a time.  The two
    256x256 kernels and gemm_tail_kernel fetch four floats per lane as one 16-byte vector: am_gemm_bf16 refuses a bias that is not
    16-byte aligned on that route (AM_ERR_INVALID, nothing launched, C untouched) instead of running a misaligned vector load.
    (2088, 72, 128): under force_big this is the shape whose 40 remainder rows go to launch_tail.
    seen (128x128 tile, bias one float into its buffer): bf16 0.41, f16 0.43 of the bound; same bits as with an aligned bias"""
    from actionmesh_amd import ops
    M, N, K = 2088, 72, 128
    a = tk._randn((M, K), 1, dev).to(dtype)
    w = tk._randn((N, K), 2, dev, 1.0 / math.sqrt(K)).to(dtype)
    buf = Arena.flat((N + 1,), torch.float32, dev)
    buf.view.copy_(tk._randn((N + 1,), 3, dev, 0.5))
    bias = buf.view[1:]
    assert bias.data_ptr() % 16 == 4
    C = Arena(M, N, dtype, dev, ld=N + 8)
    for route in ("big", "lockstep"):
        with pytest.raises(RuntimeError, match=r"status -1"):
            ops.gemm(a, w, bias=bias, out=C.view, **ROUTES[route])
        torch.cuda.synchronize()
        assert bool((C.bits == SENTINEL[dtype]).all()), f"{route}: a refused call wrote to C"
    ops.gemm(a, w, bias=bias, out=C.view, force_small=True)
    torch.cuda.synchronize()
    C.assert_untouched("C")
    buf.assert_untouched("bias buffer")
    ref, lin = tf._gemm_ref(a, w, bias, None, False)
    _check_values(C.view, ref, lin, None, K, False, "small", dtype, f"{dtype} gemm 128x128 tile, bias at 4 mod 16")
    assert torch.equal(_bits(C.view), _bits(ops.gemm(a, w, bias=bias.clone(), force_small=True)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("what", ["lda = K + 4", "C offset by 4 elements", "ldc = N + 4"])
def test_gemm_refuses_layouts_under_the_minimum(dev, dtype, what):
    """Leading dimensions are multiples of 8 elements and operands 16-byte aligned: anything less is refused with AM_ERR_INVALID before
    a kernel is launched - C, view and guards alike, still holds nothing but sentinels."""
    from actionmesh_amd import ops
    M, N, K = 37, 72, 128
    a = tk._randn((M, K), 1, dev).to(dtype)
    w = tk._randn((N, K), 2, dev, 1.0 / math.sqrt(K)).to(dtype)
    A = Arena.of(a, ld=K + 4) if what.startswith("lda") else Arena.of(a)
    C = Arena(M, N, dtype, dev, ld=N + 4 if what.startswith("ldc") else N + 8, elem_offset=4 if what.startswith("C offset") else 0)
    for route in ROUTES:
        with pytest.raises(RuntimeError, match=r"status -1"):
            ops.gemm(A.view, w, out=C.view, **ROUTES[route])
    torch.cuda.synchronize()
    assert bool((C.bits == SENTINEL[dtype]).all()), "a refused call wrote to C"
