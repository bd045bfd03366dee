"""Guard bands of the elementwise kernels (am_elementwise.hip) and of the exact-fp32 path (am_f32.hip): outputs in arenas of sentinels
(tests/_guard.py), strided inputs whose gap columns are NaN, values against fp64 at the bound each kernel's own test states, and the
same bits as the call on plain tensors."""
import math

import pytest
import torch
import torch.nn.functional as F

import test_f16_kernels_gpu as tf
import test_kernels_gpu as tk
from _guard import Arena

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = tf.DTYPES


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


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2055])
def test_f32_to_16_guards(dev, n, dtype):
    """am_f32_to_bf16: lanes convert 8 elements with one 16-byte store while `i + 8 <= n` and finish element by element: n = 1, 7 (tail
    only), 8 (one vector, no tail), 9 (vector + 1), 2055 (more than one workgroup's worth, tail of 7).  Exact: torch's conversion."""
    from actionmesh_amd import ops
    x = tk._randn((n,), n, dev) * 100
    X, Y = Arena.flat_of(x), Arena.flat((n,), dtype, dev)
    ops.f32_to_bf16(X.view, dtype=dtype, out=Y.view)
    torch.cuda.synchronize()
    X.assert_untouched("x")
    Y.assert_untouched("y")
    assert torch.equal(_bits(Y.view), _bits(x.to(dtype))) and torch.equal(_bits(Y.view), _bits(ops.f32_to_bf16(x, dtype=dtype)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [2, 256])
def test_timestep_sinusoid_guards(dev, C, dtype):
    """am_timestep_sinusoid, 3 rows, C = 2 (one frequency) and 256.  bf16: 6e-3 (test_timestep_sinusoid); float16: 2^-11 + 3e-4
    (test_point_embed_patchify_displacement_timestep_f16).  seen: bf16 0.33, f16 0.31"""
    from actionmesh_amd import ops
    t = torch.tensor([1000.0, 0.0, 523.25], device=dev)
    T, Y = Arena.flat_of(t), Arena(3, C, dtype, dev)
    ops.timestep_sinusoid(T.view, C, dtype=dtype, out=Y.view)
    torch.cuda.synchronize()
    T.assert_untouched("t")
    Y.assert_untouched("out")
    half = C // 2
    f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64, device=dev) / half)
    ref = torch.cat([torch.sin(t.double()[:, None] * f), torch.cos(t.double()[:, None] * f)], -1)
    _ratio(f"timestep_sinusoid {dtype} C={C}", (Y.view.double() - ref).abs(), torch.full_like(ref, 6e-3 if dtype == BF16 else 2.0 ** -11 + 3e-4))
    assert torch.equal(_bits(Y.view), _bits(ops.timestep_sinusoid(t, C, dtype=dtype)))


@pytest.mark.parametrize("dtype", [pytest.param(F16, id="f16"), pytest.param(BF16, id="bf16"), pytest.param(torch.float32, id="f32")])
@pytest.mark.parametrize("ld_out", [54, 64])
def test_point_embed_guards(dev, ld_out, dtype):
    """am_point_embed / am_point_embed_f32: 5 query rows of 6 channels with ld_in = 7 (the seventh column is a NaN that must not be
    read), 8 frequencies x pi -> 54 used columns: ld_out = 54 (no pad) and 64 (10 zero pad columns).  Pass-through channels and pads
    exactly; sin / cos: float16 one rounding + 1e-4 (its test), bf16 8e-3 (test_point_embed_and_displacement_kernels), fp32
    4 x 2^-24 (test_point_embed_patchify_displacement_f32).  seen: f16 0.61, bf16 0.24, f32 0.24"""
    from actionmesh_amd import ops
    rows, nf = 5, 8
    query = torch.rand((rows, 6), generator=torch.Generator().manual_seed(5)).to(dev) * 2 - 1
    Qa = Arena.of(query, ld=7)
    Y = Arena(rows, ld_out, dtype, dev)
    if dtype == torch.float32:
        ops.point_embed_f32(Qa.view, 3, 3, nf, True, ld_out=ld_out, out=Y.view)
        plain = ops.point_embed_f32(query, 3, 3, nf, True, ld_out=ld_out)
    else:
        ops.point_embed(Qa.view, 3, 3, nf, True, ld_out=ld_out, dtype=dtype, out=Y.view)
        plain = ops.point_embed(query, 3, 3, nf, True, ld_out=ld_out, dtype=dtype)
    torch.cuda.synchronize()
    Qa.assert_untouched("query")
    Y.assert_untouched("out")
    out = Y.view
    assert torch.equal(_bits(out), _bits(plain))
    fr = (math.pi * 2.0 ** torch.arange(nf, device=dev, dtype=torch.float64)).float()
    arg = (query[:, :3, None] * fr[None, None]).reshape(rows, 3 * nf).double()       # the argument is the fp32 product, as the reference forms it
    n_used = 3 + 6 * nf + 3
    assert torch.equal(out[:, :3], query[:, :3].to(dtype)) and torch.equal(out[:, 3 + 6 * nf:n_used], query[:, 3:6].to(dtype))
    assert bool((out[:, n_used:] == 0).all())
    ref = torch.cat([arg.sin(), arg.cos()], 1)
    bound = {F16: 2.0 ** -11 * ref.abs() + 1e-4, BF16: torch.full_like(ref, 8e-3), torch.float32: torch.full_like(ref, 4 * 2.0 ** -24)}[dtype]
    _ratio(f"point_embed {dtype} ld_out={ld_out}", (out[:, 3:3 + 6 * nf].double() - ref).abs(), bound)


@pytest.mark.parametrize("dtype", [pytest.param(F16, id="f16"), pytest.param(BF16, id="bf16"), pytest.param(torch.float32, id="f32")])
@pytest.mark.parametrize("ld_out", [588, 640])
def test_patchify_guards(dev, ld_out, dtype):
    """am_patchify / am_patchify_f32: 2 frames x 3 channels of 30 x 45 pixels, patch 14 -> 2 x 3 patches per frame.  Pixel rows 28, 29
    and columns 42 .. 44 belong to no patch and hold NaN: none may appear.  A gather and one rounding: exact, pad columns zero."""
    from actionmesh_amd import ops
    T, Cin, H, W, p = 2, 3, 30, 45, 14
    pix = tk._randn((T, Cin, H, W), 7, dev)
    pix[:, :, 28:] = float("nan")
    pix[:, :, :, 42:] = float("nan")
    P = Arena.flat_of(pix)
    rows = T * (H // p) * (W // p)
    Y = Arena(rows, ld_out, dtype, dev)
    if dtype == torch.float32:
        ops.patchify_f32(P.view, p, ld_out, out=Y.view)
        plain = ops.patchify_f32(pix, p, ld_out)
    else:
        ops.patchify(P.view, p, ld_out, dtype=dtype, out=Y.view)
        plain = ops.patchify(pix, p, ld_out, dtype=dtype)
    torch.cuda.synchronize()
    P.assert_untouched("pixels")
    Y.assert_untouched("out")
    ref = F.unfold(pix[:, :, :28, :42].double(), p, stride=p).transpose(1, 2).reshape(-1, Cin * p * p)
    assert not bool(torch.isnan(Y.view).any()), "a pixel outside every patch was read"
    assert torch.equal(_bits(Y.view[:, :588]), _bits(ref.to(dtype))) and bool((Y.view[:, 588:] == 0).all())
    assert torch.equal(_bits(Y.view), _bits(plain))


@pytest.mark.parametrize("dtype", [pytest.param(F16, id="f16"), pytest.param(BF16, id="bf16"), pytest.param(torch.float32, id="f32")])
def test_displacement_guards(dev, dtype):
    """am_displacement / am_displacement_f32: 5 rows of logits with ld = 8, out_dim = 3; columns 3 .. 7 are NaN and must not be read.
    bf16 1e-5 (test_point_embed_and_displacement_kernels), float16 4e-6 (its test), fp32 4 x 2^-24.  seen: bf16 0.01, f16 0.02, fp32 0.26"""
    from actionmesh_amd import ops
    lg = (tk._randn((5, 3), 9, dev) * 4).to(dtype)
    Lg = Arena.of(lg, ld=8)
    O = Arena(5, 3, torch.float32, dev)
    fn = ops.displacement_f32 if dtype == torch.float32 else ops.displacement
    fn(Lg.view, 3, O.view)
    torch.cuda.synchronize()
    Lg.assert_untouched("logits")
    O.assert_untouched("out")
    ref = 2.0 * torch.sigmoid(-lg.double()) - 1.0
    _ratio(f"displacement {dtype}", (O.view.double() - ref).abs(), torch.full_like(ref, {F16: 4e-6, BF16: 1e-5, torch.float32: 4 * 2.0 ** -24}[dtype]))
    assert torch.equal(_bits(O.view), _bits(fn(lg, 3, torch.empty((5, 3), device=dev))))


@pytest.mark.parametrize("dtype", DTYPES)
def test_flow_step_guards(dev, dtype):
    """am_flow_step on T x N x D = 3 x 7 x 13 = 273 elements (one full workgroup + 17 lanes): latents guarded, the observed frame
    bit-identical, the others at test_flow_step's 1e-6 of the rounding chain restated in fp64 (every 16-bit operation rounded to the
    type; the products and sums of 16-bit values are exact in fp64, so one rounding each, as the kernel's fp32).  seen: 0.12"""
    from actionmesh_amd import ops
    T, N, D = 3, 7, 13
    v = tk._randn((2, T, N, D), 1, dev).to(dtype)
    lat0 = tk._randn((T, N, D), 2, dev)
    V, Lt = Arena.flat_of(v), Arena.flat_of(lat0)
    ops.flow_step(V.view, Lt.view, [7.5], 0.0356, True, [True, False, True])
    plain = lat0.clone()
    ops.flow_step(v, plain, [7.5], 0.0356, True, [True, False, True])
    torch.cuda.synchronize()
    V.assert_untouched("v")
    Lt.assert_untouched("latents")
    rd = lambda x: x.float().to(dtype).double()
    v0, v1 = v[0].double(), v[1].double()
    s, dt = float(torch.tensor(7.5, dtype=torch.float32)), float(torch.tensor(0.0356, dtype=torch.float32))
    agg = rd(v0 + rd(s * rd(v1 - v0)))
    ref = lat0.double() + rd(dt * agg)
    assert torch.equal(Lt.view[1], lat0[1]), "the observed frame changed"
    _ratio(f"flow_step {dtype}", (Lt.view.double() - ref).abs()[[0, 2]], torch.full_like(ref[[0, 2]], 1e-6))
    assert torch.equal(_bits(Lt.view), _bits(plain))


# ==========================================================================================================================================
# exact-fp32 path
# ==========================================================================================================================================
@pytest.mark.parametrize("epi", ["bias", "gelu", "alias"])
@pytest.mark.parametrize("M,N,K", [(1, 8, 64), (129, 136, 100)])
def test_gemm_f32_guards_and_leading_dimensions(dev, M, N, K, epi):
    """am_gemm_f32 with lda, ldw, ldc, ldr all padded by 4 floats (the API minimum: 16-byte rows) at (1, 8, 64) and (129, 136, 100) -
    one row and 8 columns past the 128 x 128 tile, and a K slice of 4 behind three of 32; bias, erf-GELU, and the residual aliasing the
    output.  test_gemm_f32_against_fp64's bound: 1e-6 sum|a w| + 2^-22 |c|.  seen: 0.16"""
    from actionmesh_amd import ops
    g = torch.Generator().manual_seed(M + N + K)
    a = (torch.rand((M, K), generator=g) * 2 - 1).to(dev)
    w = (torch.rand((N, K), generator=g) * 2 - 1).to(dev)
    bias = torch.randn((N,), generator=g).to(dev)
    R = (torch.randn((M, N), generator=g) * 4).to(dev) if epi == "alias" else None
    gelu = epi == "gelu"
    A, W = Arena.of(a, ld=K + 4), Arena.of(w, ld=K + 4)
    C = Arena(M, N, torch.float32, dev, ld=N + 4)
    if R is not None:
        C.view.copy_(R)
        plain = R.clone()
        ops.gemm_f32(a, w, bias=bias, residual=plain, out=plain)
    else:
        plain = ops.gemm_f32(a, w, bias=bias, gelu=gelu)
    ops.gemm_f32(A.view, W.view, bias=bias, residual=C.view if R is not None else None, gelu=gelu, out=C.view)
    torch.cuda.synchronize()
    for nm, ar in (("C", C), ("A", A), ("W", W)):
        ar.assert_untouched(f"gemm_f32 {M}x{N}x{K} {epi}: {nm}")
    a64, w64 = a.double(), w.double()
    ref = a64 @ w64.T + bias.double()
    mag = a64.abs() @ w64.abs().T + bias.double().abs()
    if gelu:
        ref = F.gelu(ref)
    if R is not None:
        ref = ref + R.double()
    _ratio(f"gemm_f32 {M}x{N}x{K} {epi}", (C.view.double() - ref).abs(), 1e-6 * mag + 2.0 ** -22 * ref.abs())
    assert torch.equal(_bits(C.view), _bits(plain))


def test_gemm_f32_residual_in_its_own_arena(dev):
    """am_gemm_f32 with the residual in an arena of its own: ldr = N + 4 beside ldc = N + 4, R unchanged afterwards.  seen: 0.19"""
    from actionmesh_amd import ops
    g = torch.Generator().manual_seed(3)
    M, N, K = 129, 136, 100
    a, w = (torch.rand((M, K), generator=g) * 2 - 1).to(dev), (torch.rand((N, K), generator=g) * 2 - 1).to(dev)
    R = (torch.randn((M, N), generator=g) * 4).to(dev)
    A, W, Ra, C = Arena.of(a, ld=K + 4), Arena.of(w, ld=K + 4), Arena.of(R, ld=N + 4), Arena(M, N, torch.float32, dev, ld=N + 4)
    ops.gemm_f32(A.view, W.view, residual=Ra.view, out=C.view)
    torch.cuda.synchronize()
    for nm, ar in (("C", C), ("A", A), ("W", W), ("R", Ra)):
        ar.assert_untouched(f"gemm_f32 residual: {nm}")
    ref = a.double() @ w.double().T + R.double()
    _ratio("gemm_f32 residual", (C.view.double() - ref).abs(), 1e-6 * (a.double().abs() @ w.double().abs().T) + 2.0 ** -22 * ref.abs())
    assert torch.equal(_bits(C.view), _bits(ops.gemm_f32(a, w, residual=R))) and torch.equal(Ra.view, R)


@pytest.mark.parametrize("D", [64, 128])
def test_attention_f32_padded_rows(dev, D):
    """am_attention_f32 writing O (nseq * sq, heads * D) with ldo = heads * D + 4, from q and a packed [to_k | to_v] operand whose rows
    are padded by 4 floats too: (3, 2, 65, 33) - one partial 128-row query block per sequence, one full and one 1-key block of 32 keys.
    test_attention_f32_against_fp64's bound: rel-L2 <= 2e-6, max-abs <= 1e-5 max|V|.  seen: rel-L2 0.16, max-abs 0.02"""
    from actionmesh_amd import ops
    g = torch.Generator().manual_seed(D)
    nseq, H, sq, sk = 3, 2, 65, 33
    q2 = torch.randn((nseq * sq, H * D), generator=g).to(dev)
    kv = torch.randn((nseq * sk, H * 2 * D), generator=g).to(dev)
    Qa, KV = Arena.of(q2, ld=H * D + 4), Arena.of(kv, ld=H * 2 * D + 4)
    O = Arena(nseq * sq, H * D, torch.float32, dev, ld=H * D + 4)
    kw = dict(q_hs=D, k_hs=2 * D, v_hs=2 * D, v_off=D)
    ops.attention_f32(Qa.view, KV.view, KV.view, H, sq, sk, D, out=O.view, **kw)
    plain = ops.attention_f32(q2, kv, kv, H, sq, sk, D, **kw)
    torch.cuda.synchronize()
    for nm, ar in (("O", O), ("q", Qa), ("kv", KV)):
        ar.assert_untouched(f"attention_f32 D={D}: {nm}")
    q = q2.view(nseq, sq, H, D).transpose(1, 2).double()
    kvh = kv.view(nseq, sk, H, 2, D).double()
    k, v = kvh[:, :, :, 0].transpose(1, 2), kvh[:, :, :, 1].transpose(1, 2)
    ref = (torch.softmax((q @ k.transpose(-1, -2)) * D ** -0.5, -1) @ v).transpose(1, 2).reshape(nseq * sq, H * D)
    r, mx = tf._rel(O.view, ref) / 2e-6, float((O.view.double() - ref).abs().max()) / (1e-5 * float(v.abs().max()))
    print(f"attention_f32 D={D} padded ldo: rel-L2 / bound {r:.3f}, max-abs / bound {mx:.3f}")
    assert r <= 1.0 and mx <= 1.0
    assert torch.equal(_bits(O.view), _bits(plain))
