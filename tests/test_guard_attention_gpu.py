"""Guard bands and output leading dimensions of the attention entry points (am_attention_bf16 in both builds, am_attention_fp8 and its
quantiser): every kernel of the dispatch writes O[row][h * 128 .. + 128) of its nseq * sq rows and nothing else - with 16-byte stores
where ldo and O allow them, 8-byte stores at the API minimum (ldo % 4 == 0, O 8-byte aligned) - and reads nothing outside Q, K, V^T.

Q, K, V^T sit in flat arenas (tests/_guard.py; their pads are zero, as DESIGN.md requires), O in a row arena under three layouts:
natural, ldo = H * 128 + 8, and ldo = H * 128 + 4 with O four elements past a 16-byte boundary.  Each case asserts (a) guards and gaps
untouched, (b) values against fp64 softmax attention at the kernels' own tolerance (`_attn_close`: rel-L2 <= 1e-2 for bf16,
F16_ATTN_TOL for float16, max-abs <= 0.25 x rms; the fp8 test's 6e-2 / 0.12), (c) the same bits as the call with a plain output."""
import pytest
import torch

import test_f16_kernels_gpu as tf
import test_kernels_gpu as tk
from _guard import SENTINEL, Arena

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = tf.DTYPES
TOL = {BF16: 1e-2, F16: tf.F16_ATTN_TOL}
LAYOUTS = {"natural": (0, 0), "ldo+8": (8, 0), "ldo+4,O+4": (4, 4)}        # (row padding, element offset of O)


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


def _ref64(q, k, v):
    """fp64 softmax attention of (nseq, H, s, 128) operands -> (nseq * sq, H * 128)."""
    nseq, H, sq, _ = q.shape
    s = (q.double() @ k.double().transpose(-1, -2)) * (128 ** -0.5)
    return (torch.softmax(s, dim=-1) @ v.double()).permute(0, 2, 1, 3).reshape(nseq * sq, H * 128)


def _operands(dev, dtype, nseq, H, sq, sk, nchunks=1):
    """q, k, v and their kernel layouts inside flat arenas (pads zero, guards poisoned)."""
    q, k, v = tf._qkv(dev, nseq, H, sq, sk * nchunks, dtype)
    Q, K, Vt, skc = tk._layout(q, k, v, nchunks)
    assert skc == sk
    return q, k, v, Arena.flat_of(Q), Arena.flat_of(K), Arena.flat_of(Vt)


def _out_arena(dev, dtype, rows, H, layout):
    pad, off = LAYOUTS[layout]
    return Arena(rows, H * 128, dtype, dev, ld=H * 128 + pad, elem_offset=off)


# (nseq, H, sq, sk, dispatch codes): what each reaches is in the docstring below
ONE_PASS = [pytest.param(3, 2, 70, 17, (8,), id="short-stream"), pytest.param(1, 2, 300, 300, (98,), id="8-wave"),
            pytest.param(1, 2, 300, 1040, (68, 28), id="4x64"), pytest.param(16, 8, 1000, 257, (8,), id="resident"),
            pytest.param(1, 1, 2064, 4097, (8,), id="split-tail")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nseq,H,sq,sk,defers", ONE_PASS)
def test_attention_output_guards(dev, nseq, H, sq, sk, defers, dtype):
    """(3, 2, 70, 17) defer 8: the short-stream geometry (two 4-wave workgroups), one partial query block and one partial key tile;
    (1, 2, 300, 300) defer 98: the forced 8-wave kernel; (1, 2, 300, 1040) defer 68 / 28: the 4 waves x 64 rows kernel, lazy and exact
    re-base; (16, 8, 1000, 257) defer 8: the resident key stream (512 query blocks: eligible), which needs 16-byte output rows and must
    step aside under the ldo + 4 layout - there the bits are those of the streaming geometry (defer 58) on a plain output;
    (1, 1, 2064, 4097) defer 8: 9 query blocks with a 16-row tail, 65 key tiles = 33 supers, so the tail is cut over the key range
    and attn_combine_kernel writes its 16 rows.
    seen: rel-L2 / tolerance bf16 <= 0.28, f16 <= 0.18"""
    from actionmesh_amd import ops
    q, k, v, Q, K, Vt = _operands(dev, dtype, nseq, H, sq, sk)
    ref = _ref64(q, k, v)
    resident = (nseq, H, sq, sk) == (16, 8, 1000, 257)
    for defer in defers:
        base = ops.attention(Q.view, K.view, Vt.view, sq, sk, defer_log2=defer)
        streamed = ops.attention(Q.view, K.view, Vt.view, sq, sk, defer_log2=58) if resident else None
        for layout in LAYOUTS:
            O = _out_arena(dev, dtype, nseq * sq, H, layout)
            ops.attention(Q.view, K.view, Vt.view, sq, sk, out=O.view, defer_log2=defer)
            torch.cuda.synchronize()
            what = f"{dtype} attention ({nseq}, {H}, {sq}, {sk}) defer {defer} {layout}"
            for nm, ar in (("O", O), ("Q", Q), ("K", K), ("V^T", Vt)):
                ar.assert_untouched(f"{what}: {nm}")
            r = tk._attn_close(O.view, ref, what, rel_tol=TOL[dtype])
            print(f"{what}: rel-L2 / tolerance {r / TOL[dtype]:.3f}")
            want = streamed if (resident and layout == "ldo+4,O+4") else base
            bad = _bits(O.view) != _bits(want)
            assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ from the plain-output call, first at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_attention_two_pass_guards(dev, layout, dtype):
    """The two-pass form at (1, 1, 2320, 1100), three key chunks: pass 1 (rows = 1, state_mode 1) writes the (O, m, l) of the 9 full
    query blocks into `state` - a guarded fp32 arena - and NOTHING into the output (every element of the output arena, view included,
    still holds the sentinel); pass 2 resumes over the other chunks, rows = 2 runs the 16-row last block.  Every rank's chunk order.
    seen: rel-L2 / tolerance bf16 0.28, f16 0.18"""
    from actionmesh_amd import ops
    nseq, H, sq, skc, P = 1, 1, 2320, 1100, 3
    q, k, v, Q, K, Vt = _operands(dev, dtype, nseq, H, sq, skc, P)
    ref = _ref64(q, k, v)
    plain = tf._two_pass(ops, Q.view, K.view, Vt.view, sq, skc, P, dtype)
    for r in range(P):
        S = Arena.flat((nseq * H, Q.view.shape[2], ops.STATE_LD), torch.float32, dev)
        O = _out_arena(dev, dtype, nseq * sq, H, layout)
        what = f"{dtype} two-pass rank {r} {layout}"
        ops.attention(Q.view, K.view, Vt.view, sq, skc, out=O.view, nchunks=1, rows=1, state_mode=1, state=S.view, chunk_first=r, chunk_total=P)
        torch.cuda.synchronize()
        assert bool((O.bits == SENTINEL[dtype]).all()), f"{what}: the first pass wrote to the output"
        S.assert_untouched(f"{what}: state after pass 1")
        ops.attention(Q.view, K.view, Vt.view, sq, skc, out=O.view, nchunks=P - 1, rows=1, state_mode=2, state=S.view,
                      chunk_first=(r + 1) % P, chunk_total=P)
        ops.attention(Q.view, K.view, Vt.view, sq, skc, out=O.view, nchunks=P, rows=2)
        torch.cuda.synchronize()
        for nm, ar in (("O", O), ("state", S), ("Q", Q), ("K", K), ("V^T", Vt)):
            ar.assert_untouched(f"{what}: {nm}")
        rl = tk._attn_close(O.view, ref, what, rel_tol=TOL[dtype])
        print(f"{what}: rel-L2 / tolerance {rl / TOL[dtype]:.3f}")
        assert torch.equal(_bits(O.view), _bits(plain[r])), f"{what}: differs from the plain-output sequence"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ablate", [0, 400])
@pytest.mark.parametrize("nseq,H,sq,sk", [pytest.param(2, 2, 300, 257, id="short"), pytest.param(1, 1, 2064, 4097, id="split-tail")])
def test_attention_fp8_guards(dev, nseq, H, sq, sk, ablate, dtype):
    """am_attention_quantize_fp8 + am_attention_fp8: q8, k8, vt8 in guarded uint8 arenas, O under the three layouts; the exact-exp2
    form and `fp8_fast` (ablate 400; on the short stream it runs the exact form).  Tolerance of test_attention_fp8.py against fp64:
    rel-L2 < 6e-2 and max error < 0.12 max|ref| (fp8_fast: 6.5e-2, 0.13).
    seen: rel-L2 / tolerance <= 0.88 (both types), max error / bound <= 0.86 (bf16), 0.71 (f16)"""
    from actionmesh_amd import ops
    q, k, v, Q, K, Vt = _operands(dev, dtype, nseq, H, sq, sk)
    ref = _ref64(q, k, v)
    rel_tol, mx_tol = (6.5e-2, 0.13) if ablate == 400 else (6e-2, 0.12)
    base = ops.attention_fp8(Q.view, K.view, Vt.view, sq, sk, ablate=ablate)
    q8b, k8b, vt8b = ops.attention_fp8.last_quantized
    for layout in LAYOUTS:
        Q8, K8, V8 = (Arena.flat(t.shape, torch.uint8, dev) for t in (Q.view, K.view, Vt.view))
        O = _out_arena(dev, dtype, nseq * sq, H, layout)
        ops.attention_fp8(Q.view, K.view, Vt.view, sq, sk, out=O.view, ablate=ablate, quantize_out=(Q8.view, K8.view, V8.view))
        torch.cuda.synchronize()
        what = f"{dtype} fp8 attention ({nseq}, {H}, {sq}, {sk}) ablate {ablate} {layout}"
        for nm, ar in (("O", O), ("q8", Q8), ("k8", K8), ("vt8", V8), ("Q", Q), ("K", K), ("V^T", Vt)):
            ar.assert_untouched(f"{what}: {nm}")
        got = O.view.double()
        assert bool(torch.isfinite(got).all())
        r = float((got - ref).norm() / ref.norm()) / rel_tol
        mx = float((got - ref).abs().max() / ref.abs().max()) / mx_tol
        print(f"{what}: rel-L2 / tolerance {r:.3f}, max error / bound {mx:.3f}")
        assert r < 1.0 and mx < 1.0
        assert torch.equal(_bits(O.view), _bits(base)), f"{what}: differs from the plain-output call"
        # the quantiser fills the valid rows / columns; what it leaves of the pads is its own business, the valid part is not
        assert torch.equal(K8.view[..., :sk, :], k8b[..., :sk, :]) and torch.equal(Q8.view[:, :, :sq], q8b[:, :, :sq])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("what", ["ldo = H * 128 + 2", "O offset by 2 elements"])
@pytest.mark.parametrize("fp8", [False, True], ids=["16-bit", "fp8"])
def test_attention_refuses_outputs_under_the_minimum(dev, fp8, what, dtype):
    """Output rows are stored 8 bytes at a time at least: ldo % 4 == 0 and O 8-byte aligned, or the call is refused with
    AM_ERR_INVALID before anything is launched - the output arena, view and guards alike, holds nothing but sentinels."""
    from actionmesh_amd import ops
    nseq, H, sq, sk = 1, 2, 70, 17
    q, k, v, Q, K, Vt = _operands(dev, dtype, nseq, H, sq, sk)
    O = Arena(nseq * sq, H * 128, dtype, dev, ld=H * 128 + (2 if what.startswith("ldo") else 4), elem_offset=0 if what.startswith("ldo") else 2)
    quant = None
    if fp8:             # quantise in a valid call first, so that the refused one is the attention entry point itself
        ops.attention_fp8(Q.view, K.view, Vt.view, sq, sk)
        quant = ops.attention_fp8.last_quantized
    with pytest.raises(RuntimeError, match=r"status -1"):
        if fp8:
            ops.attention_fp8(Q.view, K.view, Vt.view, sq, sk, out=O.view, quantized=quant)
        else:
            ops.attention(Q.view, K.view, Vt.view, sq, sk, out=O.view)
    torch.cuda.synchronize()
    assert bool((O.bits == SENTINEL[dtype]).all()), "a refused call wrote to the output"
