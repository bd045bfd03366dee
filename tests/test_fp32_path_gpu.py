"""The exact-fp32 matrix path (csrc/am_f32.hip: v_mfma_f32_32x32x2_f32, fp32 operands and accumulation) and the two modules that use
it: HipAutoencoder(cross_fp32=True) - what the reference runs with autocast off in Stage II (temporal_autoencoder.py:240-243, 266-267) -
and HipImageEncoder(dtype="float32") - the DINOv2 encoder the reference runs in fp32 (pipeline.py:665-667).

Bounds come from the fp32 error model: a k-ordered fp32 fmaf chain is within ~1e-7 * K^(1/2..1) * sum|a w| of the exact product.
Every check computes its yardstick in fp64 (on the device for the large kernel cases) and prints what it measured."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---- am_gemm_f32 ---------------------------------------------------------------------------------------------------------------
def _gemm_check(M, N, K, epi, seed=0):
    from actionmesh_amd import ops
    g = _gen(seed)
    a = torch.rand((M, K), generator=g, device=DEV) * 2 - 1
    w = torch.rand((N, K), generator=g, device=DEV) * 2 - 1
    bias = torch.randn((N,), generator=g, device=DEV) if epi in ("bias", "gelu", "residual", "alias") else None
    R = torch.randn((M, N), generator=g, device=DEV) * 4 if epi in ("residual", "alias") else None
    gelu = epi == "gelu"
    if epi == "alias":
        out = R.clone()
        c = ops.gemm_f32(a, w, bias=bias, residual=out, out=out)
    else:
        c = ops.gemm_f32(a, w, bias=bias, residual=R, gelu=gelu)
    torch.cuda.synchronize()
    a64, w64 = a.double(), w.double()
    ref = a64 @ w64.T
    mag = a64.abs() @ w64.abs().T
    if bias is not None:
        ref = ref + bias.double()
        mag = mag + bias.double().abs()
    if gelu:
        ref = F.gelu(ref)
    if R is not None:
        ref = ref + R.double()
    bound = 1e-6 * mag + 2.0 ** -22 * ref.abs()
    err = (c.double() - ref).abs()
    worst = float((err / bound).max())
    print(f"gemm_f32 M={M} N={N} K={K} {epi}: max abs err {float(err.max()):.3e}, max err / bound {worst:.3f}, "
          f"max err / sum|aw| {float((err / mag).max()):.3e}")
    assert c.shape == (M, N) and bool(torch.isfinite(c).all())
    assert worst <= 1.0, worst


SHAPES = [(M, N, K) for M in (1, 37, 2000, 4113) for N in (8, 1024, 4096) for K in (64, 640, 1024, 4096)]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_f32_against_fp64(M, N, K):
    """Every (M, N, K) of the grid, plain product: per element |c - exact| <= 1e-6 sum_k |a_ik w_jk| + 2^-22 |c_ij|."""
    _gemm_check(M, N, K, "none", seed=M * 7 + N * 3 + K)


@pytest.mark.parametrize("epi", ["bias", "gelu", "residual", "alias"])
@pytest.mark.parametrize("M,N,K", [(1, 8, 64), (37, 1024, 640), (2000, 4096, 1024), (4113, 1024, 4096)])
def test_gemm_f32_epilogues(M, N, K, epi):
    """bias, exact erf-GELU (F.gelu), residual, and the residual aliasing C (the in-place fp32 stream update); |bias| joins the
    magnitude term of the bound."""
    _gemm_check(M, N, K, epi, seed=11 + M + N + K)


def test_gemm_f32_is_deterministic_across_runs_and_libraries():
    """The same call twice, and from the float16 build of the library: bit-identical (no split-K, no atomics)."""
    from actionmesh_amd import ops
    g = _gen(5)
    a = torch.randn((2000, 1024), generator=g, device=DEV)
    w = torch.randn((4096, 1024), generator=g, device=DEV)
    b = torch.randn((4096,), generator=g, device=DEV)
    c1 = ops.gemm_f32(a, w, bias=b, gelu=True)
    c2 = ops.gemm_f32(a, w, bias=b, gelu=True)
    c3 = ops.gemm_f32(a, w, bias=b, gelu=True, kind="f16")
    torch.cuda.synchronize()
    print("gemm_f32 re-run / f16-library differences:", int((c1 != c2).sum()), int((c1 != c3).sum()))
    assert torch.equal(c1, c2) and torch.equal(c1, c3)


# ---- am_attention_f32 ----------------------------------------------------------------------------------------------------------
ATTN_CASES = [(2, 8, 2000, 2056), (16, 16, 257, 257), (3, 2, 65, 1), (1, 8, 300, 4113)]


def _attn_ref(q, k, v, scale):
    """q (nseq, H, sq, D), k / v (nseq, H, sk, D) -> (nseq * sq, H * D), fp64 softmax attention."""
    s = (q.double() @ k.double().transpose(-1, -2)) * scale
    o = torch.softmax(s, -1) @ v.double()
    nseq, H, sq, D = q.shape
    return o.transpose(1, 2).reshape(nseq * sq, H * D)


@pytest.mark.parametrize("layout", ["cross", "dinov2"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("nseq,H,sq,sk", ATTN_CASES)
def test_attention_f32_against_fp64(nseq, H, sq, sk, D, layout):
    """Operands read in place from packed projection outputs.  layout "cross": q (rows, H D), kv = [to_k | to_v] split per head as the
    reference does (K of head h at column 2 h D, V at 2 h D + D); layout "dinov2": transformers' split, h D inside each of q / k / v
    (one packed [q | k | v] tensor when sq == sk).  Bound: rel-L2 <= 2e-6, max abs <= 1e-5 max|V|.
    Per element, on operands with one correct bit pattern: tests/test_attention_f32_exact_gpu.py.
    Measured on MI355X: rel-L2 <= 1.7e-6 (D = 128, sk = 2056), 5.0e-7 at sk = 4113.  A first version failed here (2.9e-6 at
    sk = 4113, D = 128): its rescale used the unrounded m * scale while the probabilities used the rounded one, so alpha was 1 + ulp
    instead of 1 on every block and the early blocks drifted; both now use the same rounded scaled max."""
    from actionmesh_amd import ops
    g = _gen(nseq * 1000 + sq + sk + D)
    if layout == "cross":
        q2 = torch.randn((nseq * sq, H * D), generator=g, device=DEV)
        kv = torch.randn((nseq * sk, H * 2 * D), generator=g, device=DEV)
        o = ops.attention_f32(q2, kv, kv, H, sq, sk, D, q_hs=D, k_hs=2 * D, v_hs=2 * D, v_off=D)
        q = q2.view(nseq, sq, H, D).transpose(1, 2)
        kvh = kv.view(nseq, sk, H, 2, D)
        k, v = kvh[:, :, :, 0].transpose(1, 2), kvh[:, :, :, 1].transpose(1, 2)
    elif sq == sk:
        qkv = torch.randn((nseq * sq, 3 * H * D), generator=g, device=DEV)
        o = ops.attention_f32(qkv, qkv, qkv, H, sq, sk, D, q_off=0, k_off=H * D, v_off=2 * H * D)
        q, k, v = (t.reshape(nseq, sq, H, D).transpose(1, 2) for t in qkv.split(H * D, 1))
    else:
        q2 = torch.randn((nseq * sq, H * D), generator=g, device=DEV)
        kv = torch.randn((nseq * sk, 2 * H * D), generator=g, device=DEV)
        o = ops.attention_f32(q2[:, :], kv[:, : H * D], kv[:, H * D:], H, sq, sk, D)      # column-slice views
        q = q2.view(nseq, sq, H, D).transpose(1, 2)
        k, v = (t.reshape(nseq, sk, H, D).transpose(1, 2) for t in kv.split(H * D, 1))
    torch.cuda.synchronize()
    ref = _attn_ref(q, k, v, D ** -0.5)
    r, mx = _rel(o, ref), float((o.double() - ref).abs().max())
    vmax = float(v.abs().max())
    print(f"attention_f32 {layout} D={D} (nseq, H, sq, sk)=({nseq}, {H}, {sq}, {sk}): rel-L2 {r:.3e}, max abs {mx:.3e} "
          f"(bound {1e-5 * vmax:.3e})")
    assert o.shape == (nseq * sq, H * D) and bool(torch.isfinite(o).all())
    assert r <= 2e-6 and mx <= 1e-5 * vmax, (r, mx)


@pytest.mark.parametrize("D", [64, 128])
def test_attention_f32_peaky_scores(D):
    """Scaled scores up to about +-60: the exact running max keeps every exponent <= 0; the softmax is nearly one-hot per row.
    Measured on MI355X: rel-L2 1.4e-6 (D = 64), 1.9e-6 (D = 128)."""
    from actionmesh_amd import ops
    nseq, H, sq, sk = 2, 4, 300, 1100
    g = _gen(77 + D)
    q = torch.randn((nseq * sq, H * D), generator=g, device=DEV)
    k = torch.randn((nseq * sk, H * D), generator=g, device=DEV)
    v = torch.randn((nseq * sk, H * D), generator=g, device=DEV)
    qh = q.view(nseq, sq, H, D).transpose(1, 2)
    kh, vh = (t.view(nseq, sk, H, D).transpose(1, 2) for t in (k, v))
    smax = float(((qh.double() @ kh.double().transpose(-1, -2)) * D ** -0.5).abs().max())
    q = q * (60.0 / smax)
    o = ops.attention_f32(q, k, v, H, sq, sk, D)
    torch.cuda.synchronize()
    ref = _attn_ref(q.view(nseq, sq, H, D).transpose(1, 2), kh, vh, D ** -0.5)
    r, mx = _rel(o, ref), float((o.double() - ref).abs().max())
    print(f"attention_f32 peaky D={D} (max |scaled score| 60): rel-L2 {r:.3e}, max abs {mx:.3e}")
    assert r <= 2e-6 and mx <= 1e-5 * float(v.abs().max()), (r, mx)


def test_attention_f32_rejects_bad_geometry():
    from actionmesh_amd import ops
    x = torch.zeros((64, 256), device=DEV)
    with pytest.raises(ValueError):
        ops.attention_f32(x, x, x, 2, 64, 64, 96)          # head_dim
    with pytest.raises(ValueError):
        ops.attention_f32(x, x, x, 3, 64, 64, 128)         # heads past the row
    with pytest.raises(TypeError):
        ops.attention_f32(x.half(), x, x, 2, 64, 64, 128)


# ---- LayerNorm and the small fp32 ops ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C,eps", [(1, 1024, 1e-5), (4113, 1024, 1e-6), (300, 4096, 1e-5), (7, 100, 1e-5)])
def test_layernorm_f32_against_fp64(rows, C, eps):
    """Within 4 fp32 ulp of the terms y is formed from.  Measured on MI355X against a bound of 4 ulp of |w xhat| + |b| alone: up to
    15x over it, on elements at the row mean (xhat ~ 0) - the fp32 x - mean, not the kernel, sets the error there."""
    from actionmesh_amd import ops
    g = _gen(rows + C)
    x = torch.randn((rows, C), generator=g, device=DEV) * 3 + 0.5
    w = torch.randn((C,), generator=g, device=DEV)
    b = torch.randn((C,), generator=g, device=DEV)
    y = ops.layernorm_f32(x, w, b, eps=eps)
    torch.cuda.synchronize()
    xh = F.layer_norm(x.double(), (C,), None, None, eps)
    ref = xh * w.double() + b.double()
    # x - mean is formed in fp32: its error is relative to |x| + |mean|, not to the difference (elements at the mean have xhat ~ 0)
    mean, rstd = x.double().mean(-1, keepdim=True), 1.0 / (x.double().var(-1, unbiased=False, keepdim=True) + eps).sqrt()
    bound = 2.0 ** -21 * (w.double().abs() * (x.double().abs() + mean.abs()) * rstd + b.double().abs())
    worst = float(((y.double() - ref).abs() / bound).max())
    print(f"layernorm_f32 rows={rows} C={C}: max err / (4 ulp of |w| (|x| + |mean|) rstd + |b|) {worst:.3f}")
    assert worst <= 1.0


def test_point_embed_patchify_displacement_f32():
    from actionmesh_amd import ops
    g = _gen(3)
    # point embedding: [x | sin(x 2^j) | cos(x 2^j) | extra | 0]; the argument is the fp32 product, as the reference forms it
    q = torch.rand((5000, 6), generator=g, device=DEV) * 2 - 1
    for include_pi in (False, True):
        e = ops.point_embed_f32(q, 3, 3, 8, include_pi, 64)
        freqs = 2.0 ** torch.arange(8, dtype=torch.float32, device=DEV)
        if include_pi:
            freqs = freqs * torch.pi
        arg = (q[:, :3, None] * freqs).reshape(5000, 24).double()
        ref = torch.cat([q[:, :3].double(), arg.sin(), arg.cos(), q[:, 3:].double(), torch.zeros((5000, 64 - 54), dtype=torch.float64,
                                                                                                    device=DEV)], 1)
        err = float((e.double() - ref).abs().max())
        print(f"point_embed_f32 include_pi={include_pi}: max abs err {err:.3e}")
        assert e.dtype == torch.float32 and err <= 4 * 2.0 ** -24
    # patchify: an exact copy
    pix = torch.randn((2, 3, 56, 42), generator=g, device=DEV)
    pt = ops.patchify_f32(pix, 14, 640)
    ref = F.unfold(pix, 14, stride=14).transpose(1, 2).reshape(-1, 3 * 14 * 14)
    assert torch.equal(pt[:, :588], ref) and bool((pt[:, 588:] == 0).all())
    # displacement: 2 sigmoid(-logits) - 1 on fp32 logits (strided rows)
    lg = torch.randn((3000, 8), generator=g, device=DEV) * 6
    out = torch.empty((3000, 3), device=DEV)
    ops.displacement_f32(lg[:, :3], 3, out)
    ref = 2 * torch.sigmoid(-lg[:, :3].double()) - 1
    err = float((out.double() - ref).abs().max())
    print(f"displacement_f32: max abs err {err:.3e}")
    assert err <= 4 * 2.0 ** -24


@pytest.mark.parametrize("padded", [False, True], ids=["natural", "padded"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_point_embed_patchify_16bit_is_the_rounded_fp32(dtype, padded):
    """point_embed / patchify and their _f32 forms are ONE kernel template over the output type: the 16-bit form is the fp32 form
    rounded to nearest even, bit for bit, at the natural and at a padded leading dimension (finite inputs: no other conversion rule)."""
    from actionmesh_amd import ops
    g = _gen(4)
    bits = lambda t: t.view(torch.int16)
    q = torch.rand((37, 6), generator=g, device=DEV) * 2 - 1
    ld = 64 if padded else 54
    for include_pi in (False, True):
        e16, e32 = ops.point_embed(q, 3, 3, 8, include_pi, ld, dtype), ops.point_embed_f32(q, 3, 3, 8, include_pi, ld)
        assert e16.dtype == dtype and e16.shape == e32.shape == (37, ld) and bool(torch.isfinite(e32).all())
        assert torch.equal(bits(e16), bits(e32.to(dtype)))
    pix = torch.randn((2, 3, 28, 42), generator=g, device=DEV)
    ld = 640 if padded else 588
    p16, p32 = ops.patchify(pix, 14, ld, dtype), ops.patchify_f32(pix, 14, ld)
    assert p16.dtype == dtype and p16.shape == p32.shape == (2 * 2 * 3, ld)
    assert torch.equal(bits(p16), bits(p32.to(dtype)))


# ---- Stage II --------------------------------------------------------------------------------------------------------------------
def _ae_case(golden_dir):
    from oracle import autoencoder_oracle as AO
    g = np.load(os.path.join(golden_dir, "ae_arch.npz"))
    width, layers, heads, latent = (int(v) for v in g["config"])
    cfg = AO.AEConfig(width=width, num_layers=layers, num_attention_heads=heads, latent_channels=latent)
    sd = AO.synthetic_state_dict(cfg, seed=0)
    assert AO.state_dict_checksum(sd) == pytest.approx(float(g["weights_checksum"]), rel=1e-12)
    t = {k: torch.from_numpy(g[k]) for k in ("latent", "framestep", "source_alpha", "target_alphas", "query", "displacement_fp32")}
    t.update({k: float(g[k]) for k in g.files if k.startswith("ref_autocast_")})
    return cfg, sd, t


def _ae(cfg, sd, **kw):
    from actionmesh_amd.autoencoder import HipAutoencoder
    m = HipAutoencoder(width=cfg.width, num_layers=cfg.num_layers, num_attention_heads=cfg.num_attention_heads,
                       latent_channels=cfg.latent_channels, **kw)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def test_stage2_cross_block_alone_against_host_fp32(golden_dir):
    """fwd_cross_attn (temporal_autoencoder.py:152-161) at the ae_arch weights on a random fp32 kv cache of 2056 keys and 2000 embedded
    queries, against oracle.autoencoder_oracle.cross_block + norm_out / proj_out / * -1 in fp32 on the host: rel-L2 <= 1e-5."""
    from oracle import autoencoder_oracle as AO
    from conftest import host_threads
    host_threads()
    cfg, sd, _ = _ae_case(golden_dir)
    gen = torch.Generator().manual_seed(17)
    kv = torch.randn((1, 2056, cfg.width), generator=gen) * 2
    pts = torch.rand((1, 2000, 6), generator=gen) * 2 - 1
    qe = torch.cat([AO.point_embed(cfg, pts[..., :3]), pts[..., 3:]], -1)
    m = _ae(cfg, sd, cross_fp32=True)
    lg = m.fwd_cross_attn(kv.to(DEV), qe.to(DEV)).cpu()
    qh = F.linear(qe, sd["proj_query.weight"], sd["proj_query.bias"])
    h = AO.cross_block(sd, cfg, qh, kv)
    ref = F.linear(F.layer_norm(h, (cfg.width,), sd["norm_out.weight"], sd["norm_out.bias"], 1e-5), sd["proj_out.weight"],
                   sd["proj_out.bias"]) * -1
    r = _rel(lg, ref)
    print(f"Stage II cross block alone (fp32): rel-L2 vs host fp32 {r:.3e}, max abs {float((lg - ref).abs().max()):.3e}")
    assert lg.shape == (1, 2000, cfg.out_dim) and r <= 1e-5, r


def _stage2(m, t, dtype):
    with torch.autocast("cuda", dtype=dtype):
        d = m(t["latent"].to(DEV), t["framestep"], t["source_alpha"], t["target_alphas"], t["query"].to(DEV))
    torch.cuda.synchronize()
    return d.cpu()


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_stage2_cross_fp32_at_the_shipped_architecture(golden_dir, dtype):
    """The whole Stage II (ae_arch fixture: width 1024, 16 + 1 blocks, 2056 keys, 2000 vertices, 3 targets) under autocast(dtype) with
    cross_fp32=True, against the reference's fp32 displacement: rel-L2 <= 1.15 x (float16) / 1.10 x (bfloat16) the reference's own
    autocast distance, no additive term; max abs within tests/test_autoencoder.py's MX (3e-3 / 2e-2).  float16: strictly closer to the
    fixture than the same inputs with cross_fp32=False."""
    cfg, sd, t = _ae_case(golden_dir)
    tag = "f16" if dtype == "float16" else "bf16"
    ref = t["displacement_fp32"]
    ref_rel = t[f"ref_autocast_{tag}_rel"]
    d = _stage2(_ae(cfg, sd, cross_fp32=True), t, getattr(torch, dtype))
    rl, err = _rel(d, ref), float((d - ref).abs().max())
    print(f"Stage II cross_fp32, {dtype}: rel-L2 {rl:.3e} (reference autocast {ref_rel:.3e}, ratio {rl / ref_rel:.3f}), max abs {err:.3e}")
    assert d.shape == ref.shape and d.dtype == torch.float32 and bool(torch.isfinite(d).all())
    K, MX = (1.15, 3e-3) if tag == "f16" else (1.10, 2e-2)
    assert rl <= K * ref_rel and err <= MX, (rl, err)
    if tag == "f16":
        d16 = _stage2(_ae(cfg, sd, cross_fp32=False), t, torch.float16)
        rl16 = _rel(d16, ref)
        print(f"Stage II float16 with the 16-bit cross block: rel-L2 {rl16:.3e} (cross_fp32: {rl:.3e})")
        assert rl < rl16, (rl, rl16)


def test_stage2_cross_fp32_refuses_16bit_stream():
    from actionmesh_amd.autoencoder import HipAutoencoder
    with pytest.raises(ValueError, match="residual_fp32"):
        HipAutoencoder(width=256, num_layers=1, num_attention_heads=2, cross_fp32=True, residual_fp32=False)
    m = HipAutoencoder(width=256, num_layers=1, num_attention_heads=2)
    with pytest.raises(RuntimeError, match="cross_fp32"):
        m.fwd_cross_attn(torch.zeros((1, 4, 256)), torch.zeros((1, 4, m.query_dim)))


# ---- DINOv2 encoder ------------------------------------------------------------------------------------------------------------
def test_encoder_float32_vitl_against_transformers(golden_dir):
    """HipImageEncoder(dtype="float32") at ViT-L/14 (tests/golden/dinov2_vitl.npz: transformers.Dinov2Model's own fp32
    last_hidden_state): rel-L2 <= 2e-5, max abs <= 1e-3; float32 and finite.  torch.float32 is accepted the same way."""
    from oracle import dinov2_oracle as DO
    from actionmesh_amd import image_encoder as IE
    g = np.load(os.path.join(golden_dir, "dinov2_vitl.npz"))
    cfg = DO.DinoConfig()
    sd = DO.synthetic_state_dict(cfg, seed=0)
    assert DO.state_dict_checksum(sd) == pytest.approx(float(g["checksum"]), rel=1e-12)
    gen = torch.Generator().manual_seed(int(g["seed"]))
    pixels = torch.randn((int(g["frames"]), 3, int(g["side"]), int(g["side"])), generator=gen) * float(g["pixel_scale"])
    ref, stride = torch.from_numpy(g["last_hidden_state_sub"]), int(g["token_stride"])
    enc = IE.HipImageEncoder(state_dict=sd, dtype="float32").to(DEV)
    out = enc.encode_pixels(pixels.to(DEV)).cpu()
    assert out.shape == (2, 257, 1024) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    sub = out[:, ::stride]
    r, mx = _rel(sub, ref), float((sub - ref).abs().max())
    print(f"HIP DINOv2 ViT-L/14 float32: rel-L2 vs transformers fp32 {r:.3e}, max abs {mx:.3e}")
    assert r <= 2e-5 and mx <= 1e-3, (r, mx)
    enc2 = IE.HipImageEncoder(state_dict=sd, dtype=torch.float32).to(DEV)
    o16 = enc2.encode_pixels(pixels.to(DEV), out_dtype=torch.bfloat16)
    assert o16.dtype == torch.bfloat16 and torch.equal(o16.cpu(), out.to(torch.bfloat16))


@pytest.mark.parametrize("name", ["head_dim_64", "head_dim_128"])
def test_encoder_float32_tiny_cases_and_launch_counts(name):
    """The two tiny encoders of tests/test_encoder_fp32_cpu.py (head_dim 64 and 128, non-square images) on the kernels: the same bound
    against the oracle, the same launch counts."""
    from test_encoder_fp32_cpu import check_case
    check_case(name, torch.device(DEV))
