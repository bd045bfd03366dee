"""Softmax shift invariance of the attention kernels (GPU).

Adding one constant to every score of a query row must leave the row's output unchanged.  The operands put a per-row offset
through the last head channel: k[..., D - 1] = 1 on every real key (padded keys stay zero, as the layout writes them) and
q[r, D - 1] = c_r * sqrt(D), so the real scores of row r move by c_r nats while a padded key still scores exactly 0 - what a key
bias does.  c_r is chosen per row on the host so that the row maxima land on the targets of BUCKETS (octaves); one launch covers
them all (row r belongs to bucket r % len(BUCKETS)).  The reference is fp64 on the host (the device's fp64 matmul is not exact enough
for the 1e-12 self-check below), computed from the 16-bit tensors the kernel receives.

Every bucket must be finite, meet the kernel's stated tolerance against fp64, and be no worse than twice the 0-octave bucket of
the same launch plus a small floor.  A chunk's partial last key tile is where this can go wrong: a padded key that took part in
the running max and the row sum would cap every real probability of a row far below 0 at 2^max and cancel its row sum.

The second part shifts DINOv2's scores by its own key bias: a single key channel per head set to a constant, which adds
q_d * beta to every score of a row."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

D = 128
BUCKETS = (40.0, 16.0, 0.0, -8.0, -12.0, -16.0, -20.0, -24.0, -32.0, -48.0, -100.0)     # row-max targets, octaves
ZERO = BUCKETS.index(0.0)
# bucket rel-L2 <= 2 x the 0-octave bucket's + FLOOR.  Measured on MI355X with the padded keys masked: the worst bucket of a launch is
# within 1.07 x its 0-octave bucket, which is 2.6e-3 .. 2.9e-3 in bfloat16 and 3.2e-4 .. 3.6e-4 in float16 (printed per launch).  Without
# the mask, rows from about -16 octaves down were off by up to 50 x, or not finite.
FLOOR = {torch.bfloat16: 1e-3, torch.float16: 2e-4}
REL_TOL = {torch.bfloat16: 1e-2, torch.float16: 2e-3}      # the kernels' stated rel-L2 against fp32 (tests/test_kernels_gpu.py)
DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from actionmesh_amd import _lib
    from conftest import host_threads
    _lib.lib()
    _lib.lib("f16")
    host_threads()
    return torch.device("cuda:0")


def _shifted(nseq, H, sq, sk, dtype, dev, seed=0, d=D):
    """Random (q, k, v) of one head width `d` in `dtype`, k[..., d - 1] = 1, q[..., d - 1] = the per-row offset that puts the row's
    maximum score on its bucket's target.  Returns (q, q0, k, v, target): q0 = q with no offset (q0[..., d - 1] = 0)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn((nseq, H, sq, d), generator=g).to(dev)
    k = torch.randn((nseq, H, sk, d), generator=g).to(dev)
    v = torch.randn((nseq, H, sk, d), generator=g).to(dev)
    q[..., d - 1] = 0.0
    k[..., d - 1] = 1.0
    q0, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    base_max = _scores64(q0, k).amax(-1)                                                         # nats, no offset
    target = torch.tensor(BUCKETS, dtype=torch.float64)[torch.arange(sq) % len(BUCKETS)]
    c = target * math.log(2.0) - base_max                                                        # offset of every row, nats
    q = q0.clone()
    q[..., d - 1] = (c * d ** 0.5).to(dtype).to(dev)
    return q, q0, k, v, target


def _scores64(q, k):
    """fp64 q k^T / sqrt(d), on the host."""
    return (q.cpu().double() @ k.cpu().double().transpose(-1, -2)) * q.shape[-1] ** -0.5


def _ref64(q, k, v):
    """fp64 softmax(q k^T / sqrt(d)) v -> (nseq * sq, H * d), computed on the host, returned on q's device."""
    nseq, H, sq, d = q.shape
    o = torch.softmax(_scores64(q, k), -1) @ v.cpu().double()
    return o.permute(0, 2, 1, 3).reshape(nseq * sq, H * d).to(q.device)


def _reference(q, q0, k, v, target):
    """fp64 reference of the shifted operands; checks that it IS the reference of the unshifted ones, and that the row maxima
    landed on their targets."""
    ref = _ref64(q, k, v)
    ref0 = _ref64(q0, k, v)
    err = float((ref - ref0).abs().max() / ref0.abs().max())
    assert err <= 1e-12, f"the fp64 reference is not shift invariant: {err:.3e}"
    got = _scores64(q, k).amax(-1) / math.log(2.0)
    assert float((got - target).abs().max()) <= 0.5, "row maxima missed their targets"
    return ref


def _layout(q, k, v, nchunks):
    """(nseq, H, S, 128) -> the kernel operands (ops.attention's layouts, padded rows / columns zero), keys in `nchunks` chunks."""
    from actionmesh_amd import ops
    nseq, H, sq, _ = q.shape
    skc = k.shape[2] // nchunks
    sq_pad, sk_pad = ops.round_up(sq, 256), ops.round_up(skc, 64)
    Q = torch.zeros((nseq, H, sq_pad, D), dtype=q.dtype, device=q.device)
    Q[:, :, :sq] = q
    K = torch.zeros((nchunks, nseq, H, sk_pad, D), dtype=q.dtype, device=q.device)
    Vt = torch.zeros((nchunks, nseq, H, D, sk_pad), dtype=q.dtype, device=q.device)
    idx = ops.perm16_index(sk_pad, q.device)
    for c in range(nchunks):
        K[c, :, :, :skc] = k[:, :, c * skc:(c + 1) * skc]
        vp = torch.zeros((nseq, H, sk_pad, D), dtype=q.dtype, device=q.device)
        vp[:, :, :skc] = v[:, :, c * skc:(c + 1) * skc]
        Vt[c] = vp[:, :, idx].transpose(-1, -2)
    return Q, K, Vt, skc


def _buckets(out, ref, sq, what, rel_tol, floor, abs_frac=0.25):
    """Per-bucket rel-L2 / max-abs of out against ref (rows of every sequence and head grouped by r % len(BUCKETS))."""
    out, ref = out.double(), ref.double()
    assert bool(torch.isfinite(out).all()), f"{what}: {int((~torch.isfinite(out)).any(-1).sum())} rows not finite"
    rows = torch.arange(out.shape[0], device=out.device) % sq % len(BUCKETS)
    rel, mx, rms = [], [], []
    for b in range(len(BUCKETS)):
        o, r = out[rows == b], ref[rows == b]
        rel.append(float((o - r).norm() / r.norm()))
        mx.append(float((o - r).abs().max()))
        rms.append(float(r.pow(2).mean().sqrt()))
    print(f"{what}: rel-L2 per bucket " + " ".join(f"{t:+.0f}:{e:.2e}" for t, e in zip(BUCKETS, rel)))
    bound = 2.0 * rel[ZERO] + floor
    bad = [f"{t:+.0f} octaves: rel-L2 {e:.3e}, max-abs {m:.3e} (rms {s:.3e})" for t, e, m, s in zip(BUCKETS, rel, mx, rms)
           if not (e <= rel_tol and m <= abs_frac * s and e <= bound)]
    assert not bad, f"{what}: buckets off (rel tol {rel_tol}, 2 x the 0-octave bucket + {floor} = {bound:.3e}): " + "; ".join(bad)


def _check16(out, ref, sq, dtype, what):
    _buckets(out, ref, sq, f"{what} {str(dtype)[6:]}", REL_TOL[dtype], FLOOR[dtype])


# ---- part 1: the 16-bit kernels -------------------------------------------------------------------------------------------------
# (nseq, H, sq, keys per chunk, chunks, defer_log2).  Product dispatch (0 / 8): the 4-wave short stream, the resident cross-attention
# kernel, the 4x64 kernel (lazy on bfloat16, exact on float16), three chunks, the split tail (24 / 63 padded keys), a one-tile-chunk
# stream through the 4x64 kernel (tile 0 is a partial last tile); forced codes (28 / 60 / 68: 4x64, 90 / 98: 8-wave, 58: 4-wave
# geometry, 78: balanced two-phase); and keys a multiple of 64 (no padded key: passes either way).
PAD_CASES = [(2, 2, 300, 257, 1), (2, 2, 300, 65, 1), (16, 8, 1100, 257, 1), (16, 8, 1030, 144, 1), (1, 2, 520, 4097, 1),
             (1, 2, 520, 1100, 3), (1, 2, 2320, 4200, 1), (1, 1, 2432, 4097, 1)]
CASES = [c + (defer,) for c in PAD_CASES for defer in (0, 8)]
CASES += [(1, 2, 520, 1100, 1, defer) for defer in (28, 60, 68, 90, 98, 58, 78)]
CASES += [(1, 2, 512, 50, 16, defer) for defer in (60, 68)]
CASES += [(2, 2, 300, 256, 1, 8), (1, 2, 520, 1024, 1, 8)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("nseq,H,sq,skc,P,defer", CASES)
def test_attention_shift_invariance(dev, nseq, H, sq, skc, P, defer, dtype):
    from actionmesh_amd import ops
    q, q0, k, v, target = _shifted(nseq, H, sq, skc * P, dtype, dev, seed=sq + skc)
    ref = _reference(q, q0, k, v, target)
    Q, K, Vt, _ = _layout(q, k, v, P)
    out = ops.attention(Q, K, Vt, sq, skc, nchunks=P, defer_log2=defer)
    torch.cuda.synchronize()
    _check16(out, ref, sq, dtype, f"attention ({nseq}, {H}, {sq}, {skc} x {P}) defer={defer}")


# two-pass form (tests/test_kernels_gpu.py::test_attention_two_pass_matches_one_pass): the full query blocks save (O, m, l) after the
# local chunk and resume over the others in ring order.  Defer 28 on bfloat16 and 8 on float16 run the exact-deferred state kernels.
@pytest.mark.parametrize("dtype,defer", [(torch.bfloat16, 0), (torch.bfloat16, 8), (torch.bfloat16, 28),
                                         (torch.float16, 0), (torch.float16, 8)], ids=["bf16-0", "bf16-8", "bf16-28", "f16-0", "f16-8"])
@pytest.mark.parametrize("nseq,H,sq,skc,P", [(2, 2, 2320, 1100, 4), (1, 1, 2432, 1030, 3)])
def test_attention_two_pass_shift_invariance(dev, nseq, H, sq, skc, P, dtype, defer):
    from actionmesh_amd import ops
    q, q0, k, v, target = _shifted(nseq, H, sq, skc * P, dtype, dev, seed=sq + skc + 1)
    ref = _reference(q, q0, k, v, target)
    Q, K, Vt, _ = _layout(q, k, v, P)
    state = torch.full((nseq * H, Q.shape[2], ops.STATE_LD), float("nan"), device=dev)
    for r in range(P):
        out = torch.full((nseq * sq, H * D), 768.0, dtype=dtype, device=dev)
        ops.attention(Q, K, Vt, sq, skc, out=out, nchunks=1, defer_log2=defer, rows=1, state_mode=1, state=state,
                      chunk_first=r, chunk_total=P)
        ops.attention(Q, K, Vt, sq, skc, out=out, nchunks=P - 1, defer_log2=defer, rows=1, state_mode=2, state=state,
                      chunk_first=(r + 1) % P, chunk_total=P)
        ops.attention(Q, K, Vt, sq, skc, out=out, nchunks=P, defer_log2=defer, rows=2)
        torch.cuda.synchronize()
        assert not (out.float() == 768.0).any(), f"rank {r}: rows left unwritten"
        _check16(out, ref, sq, dtype, f"two-pass ({nseq}, {H}, {sq}, {skc} x {P}) defer={defer} rank {r}")


# ---- controls: the fp8 and fp32 kernels mask their padded keys already -----------------------------------------------------------
@pytest.mark.parametrize("form", [0, 400], ids=["exact", "exponent_field"])
@pytest.mark.parametrize("nseq,H,sq,sk", [(2, 2, 300, 257), (1, 2, 520, 4097)])
def test_attention_fp8_shift_invariance(dev, nseq, H, sq, sk, form):
    """Tolerance: tests/test_attention_fp8.py (rel-L2 6e-2 exact, 6.5e-2 exponent field, against fp32)."""
    from actionmesh_amd import ops
    q, q0, k, v, target = _shifted(nseq, H, sq, sk, torch.bfloat16, dev, seed=sq + sk + 2)
    ref = _reference(q, q0, k, v, target)
    Q, K, Vt, _ = _layout(q, k, v, 1)
    out = ops.attention_fp8(Q, K, Vt, sq, sk, ablate=form)
    torch.cuda.synchronize()
    _buckets(out, ref, sq, f"attention_fp8 ({nseq}, {H}, {sq}, {sk}) form={form}", 6.5e-2 if form else 6e-2, 1e-2, abs_frac=1.0)


@pytest.mark.parametrize("d", [64, 128])
def test_attention_f32_shift_invariance(dev, d):
    """am_attention_f32 (exact fp32, tests/test_fp32_path_gpu.py: rel-L2 <= 2e-6 against fp64 at ordinary scores).  A shift of up to
    70 nats costs fp32 scores ~|s| 2^-24 each: the floor.  Measured: 3e-7 .. 4e-7 at 0 octaves, 2.2e-6 at -100."""
    from actionmesh_amd import ops
    nseq, H, sq, sk = 2, 4, 300, 257
    q, q0, k, v, target = _shifted(nseq, H, sq, sk, torch.float32, dev, seed=d, d=d)
    ref = _ref64(q, k, v)
    assert float((ref - _ref64(q0, k, v)).abs().max() / ref.abs().max()) <= 1e-12
    flat = lambda t, s: t.transpose(1, 2).reshape(nseq * s, H * d).contiguous()
    out = ops.attention_f32(flat(q, sq), flat(k, sk), flat(v, sk), H, sq, sk, d)
    torch.cuda.synchronize()
    _buckets(out, ref, sq, f"attention_f32 d={d}", 1e-5, 5e-6, abs_frac=1e-3)


# ---- part 2: DINOv2's key bias ----------------------------------------------------------------------------------------------------
def _dino_case():
    """ViT-L geometry, 4 layers, 2 frames (tests/test_image_encoder.py::test_hip_encoder_shipped_width_against_oracle).  In every layer
    and head one key channel d is made constant: its row of key.weight zeroed, key.bias[d] = beta.  Every key of a frame then carries
    exactly beta in channel d (any precision: beta is a power of two), so q_d * beta / sqrt(hd) is the same for all keys of a row.
    beta is the smallest power of two that puts at least 25 % of layer 0's query rows entirely at or below -24 octaves."""
    from oracle import dinov2_oracle as DO
    cfg = DO.DinoConfig(num_hidden_layers=4)
    sd = DO.synthetic_state_dict(cfg, seed=1)
    g = torch.Generator().manual_seed(5)
    pixels = torch.randn((2, 3, 224, 224), generator=g)
    C, H, hd = cfg.hidden_size, cfg.num_attention_heads, cfg.head_dim
    chan = lambda i, h: h * hd + (17 * h + 5 * i + 3) % hd
    for i in range(cfg.num_hidden_layers):
        w = sd[f"encoder.layer.{i}.attention.attention.key.weight"].clone()
        b = sd[f"encoder.layer.{i}.attention.attention.key.bias"].clone()
        for h in range(H):
            w[chan(i, h)] = 0.0
            b[chan(i, h)] = 0.0
        sd[f"encoder.layer.{i}.attention.attention.key.weight"] = w
        sd[f"encoder.layer.{i}.attention.attention.key.bias"] = b
    # layer 0's scores without the constant channel, and q in that channel
    p = "encoder.layer.0."
    h0 = DO.embeddings(sd, cfg, pixels)
    z = F.layer_norm(h0, (C,), sd[p + "norm1.weight"].float(), sd[p + "norm1.bias"].float(), cfg.layer_norm_eps)
    lin = lambda n: F.linear(z, sd[p + f"attention.attention.{n}.weight"].float(), sd[p + f"attention.attention.{n}.bias"].float())
    T, S = h0.shape[:2]
    qh, kh = (lin(n).view(T, S, H, hd).transpose(1, 2).double() for n in ("query", "key"))
    base_max = ((qh @ kh.transpose(2, 3)) * hd ** -0.5).amax(-1)                                 # (T, H, S) nats
    q_d = torch.stack([qh[:, h, :, chan(0, h) - h * hd] for h in range(H)], 1)                   # (T, H, S)
    lo = -24.0 * math.log(2.0)
    beta, frac = None, 0.0
    for e in range(0, 15):
        for sgn in (1.0, -1.0):
            f = float(((base_max + q_d * sgn * 2.0 ** e * hd ** -0.5) <= lo).double().mean())
            if f >= 0.25:
                beta, frac = sgn * 2.0 ** e, f
                break
        if beta is not None:
            break
    assert beta is not None, "no power of two up to 2^14 puts 25 % of the rows below -24 octaves"
    mx = (base_max + q_d * beta * hd ** -0.5) / math.log(2.0)                                    # octaves
    qs = torch.quantile(mx.flatten().float(), torch.tensor([0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0]))
    print(f"DINOv2 key bias beta = {beta:g}: {100 * frac:.1f} % of layer 0's rows at or below -24 octaves; row maxima (octaves) "
          "min / 10 / 25 / 50 / 75 / 90 % / max " + " / ".join(f"{x:.1f}" for x in qs.tolist()))
    sd_b = dict(sd)
    for i in range(cfg.num_hidden_layers):
        b = sd[f"encoder.layer.{i}.attention.attention.key.bias"].clone()
        for h in range(H):
            b[chan(i, h)] = beta
        sd_b[f"encoder.layer.{i}.attention.attention.key.bias"] = b
    return cfg, sd, sd_b, pixels


@pytest.fixture(scope="module")
def dino(dev):
    from oracle import dinov2_oracle as DO
    cfg, sd0, sd_b, pixels = _dino_case()
    ref0, ref_b = DO.dinov2_forward(sd0, cfg, pixels), DO.dinov2_forward(sd_b, cfg, pixels)
    return cfg, sd0, sd_b, pixels, ref0, ref_b


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_dinov2_oracle_is_key_bias_invariant(dino):
    _, _, _, _, ref0, ref_b = dino
    r = _rel(ref_b, ref0)
    print(f"DINOv2 oracle, key bias beta vs 0: rel-L2 {r:.3e}")
    assert r <= 1e-5, r


@pytest.mark.parametrize("dtype,residual_fp32", [("bfloat16", True), ("bfloat16", False), ("float16", True), ("float16", False),
                                                 ("float32", True)])
def test_hip_dinov2_key_bias_invariance(dino, dtype, residual_fp32):
    """The encoder at beta: finite, within its statement against the oracle (bfloat16 / float16: 2e-2 rel-L2, 8e-2 max abs -
    tests/test_image_encoder.py; float32: 2e-5, 1e-3 - tests/test_fp32_path_gpu.py), and as close to the encoder at 0 as two 16-bit
    runs of one function are to each other (their distances to the oracle are independent rounding: at most sqrt(2) x apart)."""
    from actionmesh_amd import image_encoder as IE
    cfg, sd0, sd_b, pixels, ref0, ref_b = dino
    kw = dict(config=dict(num_hidden_layers=cfg.num_hidden_layers), dtype=dtype, residual_fp32=residual_fp32)
    out0 = IE.HipImageEncoder(state_dict=sd0, **kw).to("cuda:0").encode_pixels(pixels.cuda()).cpu()
    out_b = IE.HipImageEncoder(state_dict=sd_b, **kw).to("cuda:0").encode_pixels(pixels.cuda()).cpu()
    assert bool(torch.isfinite(out_b).all()), "non-finite features at beta"
    r0, rb, mxb = _rel(out0, ref0), _rel(out_b, ref_b), float((out_b - ref_b).abs().max())
    d = _rel(out_b, out0)
    print(f"HIP DINOv2 {dtype} residual_fp32={residual_fp32}: rel-L2 vs oracle at 0 {r0:.3e}, at beta {rb:.3e} (max abs {mxb:.3e}); "
          f"beta vs 0 {d:.3e}")
    rel_tol, abs_tol = (2e-5, 1e-3) if dtype == "float32" else (2e-2, 8e-2)
    assert rb <= rel_tol and mxb <= abs_tol, (rb, mxb)
    assert d <= 1.5 * max(r0, rb) + (1e-6 if dtype == "float32" else 1e-4), (d, r0, rb)
