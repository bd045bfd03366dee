"""The fp8 attention where it differs from the 16-bit kernels (GPU): probabilities under the e4m3 flush, and the quantiser at the edges
of e4m3's range.

A.  One dominant key G octaves above a tail that carries a real share of the softmax mass (tests/_fp8_range.py; the fp8 twin of
    test_attention_subnormal_probabilities / test_attention_probabilities_below_half in tests/test_f16_kernels_gpu.py).  Every output
    element of every dispatch form is held to the fp64 EMULATOR of that form - which walks the tiles in the form's order, flushes what
    e4m3 flushes and divides by the form's own row sum - to output rounding: _attention_exact.check with the key count, no tolerance
    of this file's own.  Inside a form's range the emulator is the plain fp64 softmax itself (asserted) and V = 1 gives 1; past it the
    measured deviation from the fp64 softmax is printed beside the share of the mass the emulator says is lost.
B.  am_attention_quantize_fp8 against torch's (x * mul).clamp(-448, 448).to(float8_e4m3fn), bit for bit: saturation, +-inf, NaN, -0,
    the e4m3 subnormals and their ties, at every lane position of both quantiser kernels; chunk walks and rows = 2.
C.  What a NaN operand does behind the quantiser, per form."""
import functools

import pytest
import torch

import _attention_exact as X
import _fp8_range as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from actionmesh_amd import _lib
    _lib.lib()
    yield torch.device("cuda:0")
    _laid_out.cache_clear()


@functools.lru_cache(maxsize=8)
def _laid_out(shape, G, where, profile):
    """The case, its operands on the device (for the quantiser-identity check) and in the kernels' bf16 layouts (V and its V = 1 twin)."""
    import test_kernels_gpu as tk          # the tests directory is on sys.path (pytest rootdir / conftest)
    cs = R.case(*shape, G, where, profile)
    P = shape[4]
    q, k, v, v1 = (t.to("cuda:0") for t in (cs.q, cs.k, cs.v, cs.v1))
    Q, K, Vt, _ = tk._layout(q.bfloat16(), k.bfloat16(), v.bfloat16(), P)
    _, _, Vt1, _ = tk._layout(q.bfloat16(), k.bfloat16(), v1.bfloat16(), P)
    return cs, (q, k, v), Q, K, {"v": Vt, "v1": Vt1}


def _hold(out, cs, twin, form, rank, what, dev):
    """One output against the emulator of its form; returns (max err / bound, lost share)."""
    v = getattr(cs, twin)
    nseq, H, sq, skc, P = cs.shape
    tiles = -(-skc // R.TILE) * (P if rank is None else 1)
    want, lost = R.emulate(cs, v, form, rank)
    soft = R.softmax_fp64(cs, v)
    inside = R.in_range(cs, form, tiles) and (rank is None or R.in_range(cs, form, tiles * (P - 1)))
    if inside:
        main = sq - R.tail_rows(sq)
        assert lost == 0.0 and torch.equal(want[:main], soft.expand(main, X.D)), f"{what}: inside the range the emulator is the fp64 softmax"
        if twin == "v1":
            assert bool((want[:main] == 1.0).all())
    else:
        dev64 = float(((out[:sq - R.tail_rows(sq), :X.D].double().cpu() - soft) / soft).abs().max())
        print(f"    {what}: deviation from the fp64 softmax {dev64:.4f}; the emulator loses {lost:.4f} of the mass")
    return X.check(out, R.full(want, cs).to(dev), skc * P, what), lost


ONE_PASS = [(shape, form, G) for shape in (R.SHAPE_LONG, R.SHAPE_SHORT) for G in R.GS for form in R.forms_of(shape)]      # a G's cases are shared


@pytest.mark.parametrize("shape,form,G", ONE_PASS)
def test_attention_fp8_under_the_e4m3_flush(dev, shape, form, G):
    """3300 keys in three chunks of 17 tiles + 12 keys (product, 4 x 64, 8-wave and fast kernels), and the 257-key stream on which every
    form runs the 8-wave kernel (fp8_fast bit for bit the exact form).  Dominant key first (the whole tail is exponentiated against
    it), in the middle of the last chunk, or last - in the partial tile beside the masked pad keys (nothing is flushed: what was
    accumulated is rescaled in fp32).  G = 8, 11 inside every range; 12, 14 past the fast form's; 15 the 2^-10 tie; 16 past all."""
    import test_attention_exact_gpu as TX
    from actionmesh_amd import ops
    nseq, H, sq, skc, P = shape
    for where in R.WHERE:
        for profile in R.PROFILES:
            cs, qkv, Q, K, Vt = _laid_out(shape, G, where, profile)
            for twin in ("v", "v1"):
                what = f"attention_fp8 form={form} {shape} G={G} {where} {profile} {twin}"
                out = ops.attention_fp8(Q, K, Vt[twin], sq, skc, nchunks=P, ablate=form, scale=X.SCALE)
                quant = ops.attention_fp8.last_quantized
                torch.cuda.synchronize()
                if twin == "v":
                    TX._assert_quantiser_is_the_identity(*qkv, quant, P)
                _hold(out, cs, twin, form, None, what, dev)
                if form == 400 and R.kernel_of(form, -(-skc // R.TILE) * P) == "wave8":
                    exact = ops.attention_fp8(Q, K, Vt[twin], sq, skc, nchunks=P, quantized=quant, scale=X.SCALE)
                    assert torch.equal(out, exact), "fp8_fast on a short stream runs the exact form"


def test_the_4x64_form_is_refused_on_the_short_stream(dev):
    """Why the short stream has three forms and not four (_fp8_range.forms_of): the dispatch has no 4 x 64 kernel under 8 tiles."""
    from actionmesh_amd import ops
    nseq, H, sq, skc, P = R.SHAPE_SHORT
    cs, qkv, Q, K, Vt = _laid_out(R.SHAPE_SHORT, 8, "first", "pow2")
    assert 100 not in R.forms_of(R.SHAPE_SHORT) and 100 in R.forms_of(R.SHAPE_LONG)
    with pytest.raises(RuntimeError, match="ablation code"):
        ops.attention_fp8(Q, K, Vt["v"], sq, skc, nchunks=P, ablate=100, scale=X.SCALE)


@pytest.mark.parametrize("form,G", [(form, G) for G in R.GS for form in R.FORMS])
def test_attention_fp8_two_pass_and_split_tail_under_the_e4m3_flush(dev, form, G):
    """The shape of test_attention_fp8_two_pass_and_split_tail_are_exact_to_output_rounding: the one-pass run, whose 16-row last block is
    cut 16 ways over the key range on the 8-wave kernel - each range starts from its own maximum, so only the range that holds the
    dominant key can flush anything - and every rank's two-pass view: rank r walks chunk r, saves (O, m, l), and resumes over the
    others in ring order, so which chunks are exponentiated against the dominant key depends on the rank."""
    import test_attention_exact_gpu as TX
    from actionmesh_amd import ops
    shape = R.SHAPE_TWO_PASS
    nseq, H, sq, skc, P = shape
    assert R.tail_rows(sq) == 16
    for where in R.WHERE:
        for profile in R.PROFILES:
            cs, qkv, Q, K, Vt = _laid_out(shape, G, where, profile)
            for twin in ("v", "v1"):
                what = f"attention_fp8 form={form} {shape} G={G} {where} {profile} {twin}"
                one = ops.attention_fp8(Q, K, Vt[twin], sq, skc, nchunks=P, ablate=form, scale=X.SCALE)
                quant = ops.attention_fp8.last_quantized
                torch.cuda.synchronize()
                if twin == "v":
                    TX._assert_quantiser_is_the_identity(*qkv, quant, P)
                _hold(one, cs, twin, form, None, what + " one pass + split tail", dev)
                state = torch.full((nseq * H, Q.shape[2], ops.STATE_LD), float("nan"), device=dev)
                for r in range(P):
                    out = TX._two_pass(ops.attention_fp8, Q, K, Vt[twin], sq, skc, P, r, state, torch.bfloat16, dev, quantized=quant, ablate=form)
                    _hold(out, cs, twin, form, r, what + f" two-pass rank {r}", dev)


# ---- B.  the quantiser ------------------------------------------------------------------------------------------------------------------
def _specials():
    """bf16 values at the edges of e4m3 (largest finite 448, smallest subnormal 2^-9), both signs; what they must become is torch's
    business: +-0; 448 and its bf16 neighbours 446, 450; 464 (the tie to the next binade's first value, 480) and beyond: 480, 65504,
    bf16's largest finite value, inf - all +-448; NaN; the subnormals 2^-9, 1.5 2^-10 (-> 2^-9), 3 2^-10 (tie -> 2^-8), 5 2^-10
    (tie -> 2^-8), 2^-10 (tie -> 0), 2^-11 and bf16's smallest subnormal (-> a signed zero)."""
    u = 2.0 ** -10
    pos = [0.0, 448.0, 446.0, 450.0, 464.0, 480.0, 65504.0, float(torch.finfo(torch.bfloat16).max), float("inf"), float("nan"),
           2 * u, u, 1.5 * u, 3 * u, 5 * u, 0.5 * u, 2.0 ** -133]
    sp = torch.tensor(pos + [-x for x in pos], dtype=torch.float32).bfloat16()
    f = sp.float()
    assert float(f[2]) == 446 and float(f[3]) == 450 and float(f[13]) == 3 * u and float(f[16]) == 2.0 ** -133 and float(f[6]) > 65000
    assert bool(torch.signbit(f[len(pos)])) and float(f[len(pos)]) == 0.0 and int(torch.isnan(f).sum()) == 2
    return sp


def _want(x, mul):
    """torch on the CPU: (x * mul).clamp(-448, 448) -> e4m3 bytes."""
    return (x.float().cpu() * mul).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)


def _same_bytes(got, want, what):
    got = got.cpu()
    nan = (want & 0x7F) == 0x7F
    bad = ((got != want) & ~nan) | (((got & 0x7F) == 0x7F) != nan)
    print(f"    {what}: {int(bad.sum())} of {want.numel()} bytes differ; {int(nan.sum())} NaN, {int(((want & 0x7F) == 0x7E).sum())} saturated, "
          f"{int((want == 0x80).sum())} negative zeros, {int(((want & 0x78) == 0).sum() - ((want & 0x7F) == 0).sum())} subnormal")
    assert not bool(bad.any()), f"{what}: first at {bad.nonzero()[0].tolist()}: got {int(got[bad][0]):#x}, want {int(want[bad][0]):#x}"


def _plant_rows(t, sp):
    """Special i at element `pos` of the 16-element group 16 i + pos, for every pos (quant_rows_kernel: one thread per group, element pos
    = byte pos & 3 of packed word pos >> 2), counted from the front of t's storage and, mirrored, from its back."""
    flat = t.view(-1)
    i = torch.arange(sp.numel()).repeat_interleave(16)
    pos = torch.arange(16).repeat(sp.numel())
    at = (16 * i + pos) * 16 + pos
    flat[at] = sp[i].to(flat.device)
    flat[flat.numel() - 1 - at] = sp[i].to(flat.device)


def _plant_vt(vt, sp):
    """Special i at each of the 64 positions of a V^T tile (quant_vt_kernel: one thread per (channel row, tile), perm16 / kperm gather):
    plant n = 64 i + pos goes to (channel row, tile) number n mod (rows x tiles), and each time that count wraps the position moves on
    by one, so that no two plants meet and every special still visits all 64 positions."""
    rows_t = vt.view(-1, vt.shape[-1])
    rows, tiles = rows_t.shape[0], vt.shape[-1] // 64
    assert (rows * tiles) % 64 == 0 and sp.numel() * 64 < 64 * rows * tiles
    n = torch.arange(sp.numel() * 64)
    m, wrap = n % (rows * tiles), n // (rows * tiles)
    at = (m % rows) * vt.shape[-1] + (m // rows) * 64 + (n + wrap) % 64
    assert at.unique().numel() == n.numel()
    rows_t.view(-1)[at] = sp[n // 64].to(vt.device)


def _vt_want(Vt):
    """vt8[ch][pos] = e4m3(V[kperm(pos)][ch]) from the bf16 V^T, which stores key k at its perm16 position."""
    import test_attention_exact_gpu as TX
    from actionmesh_amd import ops
    sk_pad = Vt.shape[-1]
    keyorder = Vt.cpu()[..., ops.perm16_index(sk_pad)]
    return _want(keyorder[..., TX._kperm(sk_pad)], 1.0)


def _quant_operands(nseq, H, sq, skc, chunks, dev, seed):
    from actionmesh_amd import ops
    g = torch.Generator().manual_seed(seed)
    sq_pad, sk_pad = ops.round_up(sq, 256), ops.round_up(skc, 64)
    mk = lambda *s: (torch.randn(s, generator=g) * torch.exp2(torch.randint(-12, 9, s, generator=g).float())).bfloat16()
    return mk(nseq, H, sq_pad, 128).to(dev), mk(chunks, nseq, H, sk_pad, 128).to(dev), mk(chunks, nseq, H, 128, sk_pad).to(dev)


@pytest.mark.parametrize("scale", [X.SCALE, 128 ** -0.5], ids=["mul_one", "mul_sdpa"])
def test_quantiser_is_torchs_e4m3_at_the_edges(dev, scale):
    """Every byte of q8, k8 and vt8, the pad rows included, against torch; NaNs by isnan.  The body is randn x 2^(-12 .. 8): values from
    under the smallest subnormal to over the saturation.  With scale = float32(ln 2) the Q multiplier is exactly 1 and the planted
    values meet the edges themselves; with 1 / sqrt(128) the fp32 product scale * log2 e is formed as the library forms it."""
    from actionmesh_amd import ops
    sp = _specials()
    Q, K, Vt = _quant_operands(1, 2, 300, 200, 1, dev, seed=17)
    for t in (Q, K):
        _plant_rows(t, sp)
    _plant_vt(Vt, sp)
    out = tuple(torch.full(t.shape, 0xA5, dtype=torch.uint8, device=dev) for t in (Q, K, Vt))
    ops.attention_quantize_fp8(Q, K, Vt, 300, 200, out, scale=scale)
    torch.cuda.synchronize()
    mul = torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.44269504088896340736, dtype=torch.float32)
    assert scale != X.SCALE or float(mul) == 1.0
    _same_bytes(out[1], _want(K, 1.0), "k8")
    _same_bytes(out[2], _vt_want(Vt), "vt8")
    _same_bytes(out[0], _want(Q, mul), f"q8 (mul = {float(mul)!r})")


def test_quantiser_walks_the_chunks_it_is_told_to(dev):
    """Three chunks.  chunk_first = 1, chunk_total = 3, two chunks walked: chunks 1 and 2 are written, chunk 0 keeps its sentinel.
    rows = 2 (all three chunks, in order): q8 is left untouched."""
    from actionmesh_amd import ops
    sp = _specials()
    Q, K, Vt = _quant_operands(2, 1, 70, 200, 3, dev, seed=18)
    for c in range(3):
        _plant_rows(K[c], sp)
        _plant_vt(Vt[c], sp)
    _plant_rows(Q, sp)
    mul = torch.tensor(128 ** -0.5, dtype=torch.float32) * torch.tensor(1.44269504088896340736, dtype=torch.float32)
    wq, wk, wv = _want(Q, mul), _want(K, 1.0), torch.stack([_vt_want(Vt[c]) for c in range(3)])
    out = tuple(torch.full(t.shape, 0xA5, dtype=torch.uint8, device=dev) for t in (Q, K, Vt))
    ops.attention_quantize_fp8(Q, K, Vt, 70, 200, out, nchunks=2, chunk_first=1, chunk_total=3)
    torch.cuda.synchronize()
    _same_bytes(out[0], wq, "ring walk q8")
    for c in (1, 2):
        _same_bytes(out[1][c], wk[c], f"ring walk k8 chunk {c}")
        _same_bytes(out[2][c], wv[c], f"ring walk vt8 chunk {c}")
    assert bool((out[1][0] == 0xA5).all()) and bool((out[2][0] == 0xA5).all()), "a chunk that is not walked was written"
    out = tuple(torch.full(t.shape, 0xA5, dtype=torch.uint8, device=dev) for t in (Q, K, Vt))
    ops.attention_quantize_fp8(Q, K, Vt, 70, 200, out, nchunks=3, rows=2)
    torch.cuda.synchronize()
    assert bool((out[0] == 0xA5).all()), "rows = 2 must leave q8 alone"
    _same_bytes(out[1], wk, "rows = 2 k8")
    _same_bytes(out[2], wv, "rows = 2 vt8")


# ---- C.  behind the quantiser ----------------------------------------------------------------------------------------------------------
NAN_CASES = [((1, 2, 300, 1100, 3), form) for form in R.FORMS] + [((1, 2, 300, 257, 1), 0)]


@pytest.mark.parametrize("shape,form", NAN_CASES)
def test_a_nan_operand_behind_the_quantiser(dev, shape, form):
    """Two heads, the NaN in head 1 only; head 0 must come out bit for bit as without it.
    V: a NaN at (key, channel c) makes channel c of every row of the head NaN and no other - in every form: 0 x NaN is NaN on the
       matrix pipe whatever the key's probability.
    K: a NaN anywhere in a key's row makes that key's score NaN for every query.  exp2 forms: 2^NaN = NaN reaches P and the row sum -
       every row of the head is NaN.  fp8_fast: the saturating byte convert writes 0 for a NaN score - the key silently drops out
       and the rows stay finite: exactly the emulator's output with that key's probability 0.  A stated limit of that form.
    Q: a NaN in one query row makes that row NaN and no other (fp8_fast: all its bytes are 0, and 0 / 0)."""
    import test_kernels_gpu as tk
    from actionmesh_amd import ops
    nseq, H, sq, skc, P = shape
    cs = R.case(*shape, 8, "middle", "pow2")
    kernel = R.kernel_of(form, -(-skc // R.TILE) * P)
    key, row, c = (skc if P > 1 else 0) + 70, 7, 37          # a tail key of a second tile, a query row, a channel
    assert key != cs.dom

    def run(q, k, v):
        Q, K, Vt, _ = tk._layout(q.to(dev).bfloat16(), k.to(dev).bfloat16(), v.to(dev).bfloat16(), P)
        out = ops.attention_fp8(Q, K, Vt, sq, skc, nchunks=P, ablate=form, scale=X.SCALE)
        torch.cuda.synchronize()
        return out.float().cpu()

    clean = run(cs.q, cs.k, cs.v)
    assert bool(torch.isfinite(clean).all())
    h1 = slice(X.D, 2 * X.D)

    v = cs.v.clone(); v[0, 1, key, c] = float("nan")
    out = run(cs.q, cs.k, v)
    assert torch.equal(out[:, :X.D], clean[:, :X.D]), "V: the other head changed"
    nan = torch.isnan(out[:, h1])
    print(f"    form {form} ({kernel}) NaN in V: {int(nan.sum())} NaN outputs, {int(nan[:, c].sum())} of them in channel {c}")
    assert bool(nan[:, c].all()) and int(nan.sum()) == sq and torch.equal(out[:, h1][~nan], clean[:, h1][~nan])

    k = cs.k.clone(); k[0, 1, key, 5] = float("nan")
    out = run(cs.q, k, cs.v)
    assert torch.equal(out[:, :X.D], clean[:, :X.D]), "K: the other head changed"
    nan = torch.isnan(out[:, h1])
    print(f"    form {form} ({kernel}) NaN in K: {int(nan.sum())} of {nan.numel()} outputs of the head are NaN")
    if kernel == "fast":
        s = cs.s.clone(); s[key] = float("-inf")
        want, _ = R.emulate(cs._replace(s=s), cs.v, form)
        assert not bool(nan.any()), "fp8_fast: the byte convert drops a NaN score"
        X.check(out[:, h1].bfloat16(), want, skc * P, "fp8_fast without the NaN key")
    else:
        assert bool(nan.all())

    q = cs.q.clone(); q[0, 1, row, 3] = float("nan")
    out = run(q, cs.k, cs.v)
    nan = torch.isnan(out)
    print(f"    form {form} ({kernel}) NaN in Q: {int(nan.sum())} NaN outputs, {int(nan[row, h1].sum())} of them in the row")
    assert bool(nan[row, h1].all()) and int(nan.sum()) == X.D
    assert torch.equal(out[~nan], clean[~nan])
