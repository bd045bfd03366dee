"""Every dispatch form of the bf16, f16 and fp8 attention kernels, element by element, on exact-softmax operands (GPU).

tests/_attention_exact.py: scale = float32(ln 2) makes scale * log2 e exactly 1.0f, integer operands make every score an integer and
every probability a power of two, exact in bf16, f16 and e4m3 - the kernels are left with their fp32 accumulation and the rounding of
the output, and each element must be finite and within (u_out + 4 n_keys 2^-24) |ref| of the fp64 reference (u_out = 2^-8 / 2^-11).
The whole-tensor norms of the other attention tests cannot see an error confined to a few rows (tests/test_attention_exact_cpu.py).
Shapes and forms are the smallest at which the other attention tests already reach each dispatch form; every case runs the three
score profiles, and prints its max err / bound with the (row, channel) where it stands."""
import functools

import pytest
import torch

import _attention_exact as X

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
DTYPE_IDS = ["bf16", "f16"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from actionmesh_amd import _lib
    _lib.lib()
    _lib.lib("f16")
    yield torch.device("cuda:0")
    _case.cache_clear()          # the shared operands and references go with the module


@functools.lru_cache(maxsize=6)
def _case(nseq, H, sq, sk_total, nchunks, profile, family):
    """Operands (checked against their own conditions) and the fp64 reference, on the device; shared by every form of a shape."""
    q, k, v = X.operands(nseq, H, sq, sk_total, profile, seed=sq + sk_total, family=family, nchunks=nchunks, device="cuda:0")
    return q, k, v, X.reference(q, k, v)


def _laid_out(q, k, v, nchunks, dtype):
    import test_kernels_gpu as tk          # the tests directory is on sys.path (pytest rootdir / conftest)
    return tk._layout(q.to(dtype), k.to(dtype), v.to(dtype), nchunks)


# ---- the 16-bit kernels -------------------------------------------------------------------------------------------------------------
# tests/test_kernels_gpu.py::test_attention: 0 / 8 product dispatch; 60 / 68 forced 4 waves x 64 rows (68 lazy re-base + exact fallback,
# 28 exact deferred re-base); 90 / 98 forced 8-wave kernel; 58 2 x 4-wave geometry; 78 balanced two-phase
DEFERS = [0, 8, 28, 60, 68, 90, 98, 58, 78]
SHAPES16 = [(1, 2, 300, 300, 1), (5, 2, 49, 9, 1), (1, 2, 520, 1040, 4),
            (1, 2, 2320, 4200, 1),          # 16-row last block: split-KV tail and merge
            (2, 1, 2305, 4224, 2)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("defer", DEFERS)
@pytest.mark.parametrize("nseq,H,sq,skc,P", SHAPES16)
def test_attention_is_exact_to_output_rounding(dev, nseq, H, sq, skc, P, defer, dtype):
    from actionmesh_amd import ops
    for profile in X.PROFILES:
        q, k, v, ref = _case(nseq, H, sq, skc * P, P, profile, "16bit")
        Q, K, Vt, _ = _laid_out(q, k, v, P, dtype)
        out = ops.attention(Q, K, Vt, sq, skc, nchunks=P, defer_log2=defer, scale=X.SCALE)
        torch.cuda.synchronize()
        X.check(out, ref, skc * P, f"attention {str(dtype)[6:]} defer={defer} ({nseq}, {H}, {sq}, {skc} x {P}) {profile}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("defer", [0, 8])
def test_resident_cross_attention_is_exact_to_output_rounding(dev, defer, dtype):
    """attn_resident_kernel at the cross-attention's context: four full tiles plus one key."""
    from actionmesh_amd import ops
    nseq, H, sq, sk = 16, 8, 1100, 257
    for profile in X.PROFILES:
        q, k, v, ref = _case(nseq, H, sq, sk, 1, profile, "16bit")
        Q, K, Vt, _ = _laid_out(q, k, v, 1, dtype)
        out = ops.attention(Q, K, Vt, sq, sk, defer_log2=defer, scale=X.SCALE)
        torch.cuda.synchronize()
        X.check(out, ref, sk, f"resident cross-attention {str(dtype)[6:]} defer={defer} ({nseq}, {H}, {sq}, {sk}) {profile}")


def _two_pass(attend, Q, K, Vt, sq, skc, P, r, state, dtype, dev, **kw):
    """Rank r's view, as tests/test_kernels_gpu.py::test_attention_two_pass_matches_one_pass drives it: the full query blocks attend to
    chunk r (state saved, output untouched), resume over the others in ring order, the short last block runs one pass."""
    nseq, H = Q.shape[:2]
    out = torch.full((nseq * sq, H * X.D), 768.0, dtype=dtype, device=dev)
    attend(Q, K, Vt, sq, skc, out=out, nchunks=1, rows=1, state_mode=1, state=state, chunk_first=r, chunk_total=P, scale=X.SCALE, **kw)
    assert bool((out.float() == 768.0).all()), "the first pass must not write the output"
    attend(Q, K, Vt, sq, skc, out=out, nchunks=P - 1, rows=1, state_mode=2, state=state, chunk_first=(r + 1) % P, chunk_total=P,
           scale=X.SCALE, **kw)
    attend(Q, K, Vt, sq, skc, out=out, nchunks=P, rows=2, scale=X.SCALE, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("defer", [0, 8])
def test_attention_two_pass_is_exact_to_output_rounding(dev, defer, dtype):
    """stair_up's step stands in the last chunk: ranks 0 .. P - 2 meet it in the resume pass, which must rescale the saved state; rank
    P - 1 saves it and resumes over keys that all lie far below its m_run."""
    from actionmesh_amd import ops
    nseq, H, sq, skc, P = 2, 2, 2320, 1100, 4
    for profile in X.PROFILES:
        q, k, v, ref = _case(nseq, H, sq, skc * P, P, profile, "16bit")
        if profile == "stair_up":
            assert float(k[0, 0, (P - 1) * skc, X.D_STAIR]) < float(k[0, 0, -1, X.D_STAIR]), "the step must stand in the last chunk"
        Q, K, Vt, _ = _laid_out(q, k, v, P, dtype)
        state = torch.full((nseq * H, Q.shape[2], ops.STATE_LD), float("nan"), device=dev)
        for r in range(P):
            out = _two_pass(ops.attention, Q, K, Vt, sq, skc, P, r, state, dtype, dev, defer_log2=defer)
            X.check(out, ref, skc * P, f"two-pass {str(dtype)[6:]} defer={defer} ({nseq}, {H}, {sq}, {skc} x {P}) rank {r} {profile}")


# ---- the fp8 kernels ----------------------------------------------------------------------------------------------------------------
def _kperm(n):
    """Key order of the fp8 V^T inside each 64-key tile (tests/test_attention_fp8.py)."""
    pos = torch.arange(n)
    t, p = pos // 64, pos % 64
    h, j = p >> 5, p & 31
    return t * 64 + 32 * (j >> 4) + (j & 3) + 8 * ((j & 15) >> 2) + 4 * h


def _assert_quantiser_is_the_identity(q, k, v, quant, P):
    """attention_fp8.last_quantized, decoded, IS the integer operands: q8 because scale * log2 e = 1, k8 directly, vt8 through _kperm."""
    q8, k8, vt8 = (t.view(torch.float8_e4m3fn).float() for t in quant)
    nseq, H, sq, _ = q.shape
    skc = k.shape[2] // P
    sk_pad = k8.shape[-2]
    assert torch.equal(q8[:, :, :sq], q) and not bool(q8[:, :, sq:].any()), "q8 is not Q"
    perm = _kperm(sk_pad).to(q.device)
    for c in range(P):
        assert torch.equal(k8[c, :, :, :skc], k[:, :, c * skc:(c + 1) * skc]) and not bool(k8[c, :, :, skc:].any()), "k8 is not K"
        vt = torch.zeros((nseq, H, X.D, sk_pad), device=q.device)
        vt[..., :skc] = v[:, :, c * skc:(c + 1) * skc].transpose(-1, -2)
        assert torch.equal(vt8[c], vt[..., perm]), "vt8 is not V^T in the tile order of the fp8 kernels"


# 0 product (free-running) kernel, 100 4 waves x 64 rows, 200 8-wave ping-pong kernel, 400 exponent-field probabilities (fp8_fast).
# The short stream (under 8 tiles) runs the 8-wave kernel: 400 must take the exact form there; 100 is refused by the dispatch.
FP8_CASES = [(shape, form) for shape in [(1, 2, 2320, 2320, 1), (2, 1, 300, 4111, 2), (1, 1, 256, 9 * 64 + 1, 1)] for form in (0, 100, 200, 400)]
FP8_CASES += [((2, 2, 300, 257, 1), form) for form in (0, 200, 400)]


@pytest.mark.parametrize("shape,form", FP8_CASES)
def test_attention_fp8_is_exact_to_output_rounding(dev, shape, form):
    from actionmesh_amd import ops
    nseq, H, sq, skc, P = shape
    for profile in X.PROFILES:
        q, k, v, ref = _case(nseq, H, sq, skc * P, P, profile, "fp8")
        Q, K, Vt, _ = _laid_out(q, k, v, P, torch.bfloat16)
        out = ops.attention_fp8(Q, K, Vt, sq, skc, nchunks=P, ablate=form, scale=X.SCALE)      # through the library's own quantiser
        torch.cuda.synchronize()
        _assert_quantiser_is_the_identity(q, k, v, ops.attention_fp8.last_quantized, P)
        X.check(out, ref, skc * P, f"attention_fp8 form={form} ({nseq}, {H}, {sq}, {skc} x {P}) {profile}")
        if form == 400 and skc * P < 8 * 64:
            exact = ops.attention_fp8(Q, K, Vt, sq, skc, nchunks=P, quantized=ops.attention_fp8.last_quantized, scale=X.SCALE)
            assert torch.equal(out, exact), "fp8_fast on a short stream runs the exact form"


def test_attention_fp8_two_pass_and_split_tail_are_exact_to_output_rounding(dev):
    """The smallest case of tests/test_attention_fp8.py::test_attention_fp8_two_pass_and_split_tail: every rank's two-pass view (state
    saved and resumed, the short last block split over the key range and merged), and the one-pass run that quantises the operands."""
    from actionmesh_amd import ops
    nseq, H, sq, skc, P = 2, 2, 2320, 1100, 4
    for profile in X.PROFILES:
        q, k, v, ref = _case(nseq, H, sq, skc * P, P, profile, "fp8")
        if profile == "stair_up":
            assert float(k[0, 0, (P - 1) * skc, X.D_STAIR]) < float(k[0, 0, -1, X.D_STAIR]), "the step must stand in the last chunk"
        Q, K, Vt, _ = _laid_out(q, k, v, P, torch.bfloat16)
        one = ops.attention_fp8(Q, K, Vt, sq, skc, nchunks=P, scale=X.SCALE)
        quant = ops.attention_fp8.last_quantized
        torch.cuda.synchronize()
        _assert_quantiser_is_the_identity(q, k, v, quant, P)
        X.check(one, ref, skc * P, f"attention_fp8 one pass + split tail ({nseq}, {H}, {sq}, {skc} x {P}) {profile}")
        state = torch.full((nseq * H, Q.shape[2], ops.STATE_LD), float("nan"), device=dev)
        for r in range(P):
            out = _two_pass(ops.attention_fp8, Q, K, Vt, sq, skc, P, r, state, torch.bfloat16, dev, quantized=quant)
            X.check(out, ref, skc * P, f"attention_fp8 two-pass ({nseq}, {H}, {sq}, {skc} x {P}) rank {r} {profile}")
