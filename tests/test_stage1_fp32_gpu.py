"""Exact-fp32 Stage I on the device (GPU): the two kernels of csrc/am_stage1_f32.hip against their contracts in
include/actionmesh_amd.h, HipDenoiser(dtype="float32") on the tiny fixtures (the assertions of tests/test_stage1_fp32_cpu.py, now on the
kernels) and at the headline architecture, and the use the mode is for: standing in for the reference's host fp32 forward as the
yardstick of a 16-bit run.

Bounds.  Model level: rel-L2 <= 2e-5 against the fp32 values of the reference's own modules (tests/_stage1_fp32.py).  Through the sampler
at the headline architecture: max(2e-5, ref_autocast_curve[step] / 100) - errors grow through the sampler by the same dynamics in any
precision (the reference's own bf16 curve grows 26-fold over the 30 steps); the ratio of unit roundoffs, 2^-15, predicts 1 / 30 000 of
that curve, and the factor 100 leaves room for the fp32 accumulation-order noise over K <= 4096 that the bf16 curve does not contain.
am_head_post_f32: per element 2^-20 (|y_2i| + |y_2i+1|) of the exact normalised pair - at most 7 roundings on the mean, halved through
the root, plus four for normalise, gain and the rotation: < 8 u = 2^-21, and a factor of two of headroom.  am_flow_step_f32: the bits
of the torch fp32 expression."""
import os

import numpy as np
import pytest
import torch

import _stage1_fp32 as S
from _guard import Arena

pytestmark = pytest.mark.gpu
HD = 128


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from actionmesh_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---- am_head_post_f32 ----------------------------------------------------------------------------------------------------------
# (off, head stride, row width) in units of head_dim, for `heads` heads: the packed self projection (q and k chunks of [q | k | v] per
# head), the cross-attention's to_q output and the context's [k | v] per head
LAYOUTS = {
    "self_q": lambda H: (0, 3 * HD, 3 * HD * H),
    "self_k": lambda H: (HD, 3 * HD, 3 * HD * H),
    "cross_q": lambda H: (0, HD, HD * H),
    "cross_k": lambda H: (0, 2 * HD, 2 * HD * H),
}


def _head_post_exact(x, w, off, hs, heads, cos, sin, rpf):
    """The header's contract in fp64: (out, bound) over the addressed chunks, everything else of x unchanged."""
    out = x.double().clone()
    bound = torch.zeros_like(out)
    rows = x.shape[0]
    for h in range(heads):
        c = x[:, off + h * hs: off + h * hs + HD].double()
        y = c * torch.rsqrt(c.pow(2).mean(-1, keepdim=True) + 1e-6) * w.double()
        pair = y.abs().reshape(rows, HD // 2, 2).sum(-1).repeat_interleave(2, dim=1)
        if cos is not None:
            frame = torch.arange(rows) // rpf
            cs, sn = cos.double()[frame].repeat_interleave(2, dim=1), sin.double()[frame].repeat_interleave(2, dim=1)
            yr, yi = y.reshape(rows, HD // 2, 2).unbind(-1)
            y = y * cs + torch.stack([-yi, yr], dim=-1).flatten(1) * sn
        out[:, off + h * hs: off + h * hs + HD] = y
        bound[:, off + h * hs: off + h * hs + HD] = pair * 2.0 ** -20
    return out, bound


@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_head_post_f32_against_fp64(dev, layout, rope):
    """1 row, and 5 frames of L = 3 rows (the frame changes inside the rows one workgroup handles); 1 and 3 heads; X in a poisoned arena with
    a 4-float gap behind every row, the gain and the tables in arenas of their own: a read outside an operand poisons the result, a write
    outside the addressed chunks changes a sentinel or a column that must keep its bits.  Two runs give identical bits.
    seen (max |got - exact| / bound over the cases of a layout): 0.15 .. 0.16 without tables, 0.18 .. 0.23 with them"""
    from actionmesh_amd import ops
    from actionmesh_amd.denoiser import rope_tables_host
    gen = torch.Generator().manual_seed(7)
    worst = 0.0
    for heads in (1, 3):
        for frames, rpf in ((1, 1), (5, 3)):
            rows = frames * rpf
            off, hs, width = LAYOUTS[layout](heads)
            x = torch.randn((rows, width), generator=gen) * 3.0
            w = 1.0 + 0.1 * torch.randn((HD,), generator=gen)
            cos = sin = None
            if rope:
                cos, sin = rope_tables_host(torch.arange(frames, dtype=torch.float32)[None] * 1.5 + 2.0)
            exact, bound = _head_post_exact(x, w, off, hs, heads, cos, sin, rpf)
            runs = []
            for _ in range(2):
                X = Arena.of(x.to(dev), ld=width + 4)
                Wt = Arena.flat_of(w.to(dev))
                tabs = None if not rope else (Arena.flat_of(cos.to(dev)), Arena.flat_of(sin.to(dev)))
                ops.head_post_f32(X.view, heads, Wt.view, off=off, head_stride=hs, rope=None if tabs is None else (tabs[0].view, tabs[1].view),
                                  rows_per_frame=rpf)
                torch.cuda.synchronize()
                X.assert_untouched(f"X {layout} heads={heads} rows={rows}")
                Wt.assert_untouched("w")
                assert torch.equal(Wt.view.cpu(), w)
                if tabs is not None:
                    tabs[0].assert_untouched("cos"); tabs[1].assert_untouched("sin")
                    assert torch.equal(tabs[0].view.cpu(), cos) and torch.equal(tabs[1].view.cpu(), sin)
                runs.append(X.view.cpu())
            got = runs[0]
            assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), "two runs differ"
            chunk = bound > 0
            assert torch.equal(got[~chunk].view(torch.int32), x[~chunk].view(torch.int32)), "a column outside the addressed chunks changed"
            assert torch.isfinite(got).all()
            ratio = ((got.double() - exact).abs()[chunk] / bound[chunk]).max().item()
            worst = max(worst, ratio)
            assert ratio <= 1.0, (layout, rope, heads, rows, ratio)
    print(f"head_post_f32 {layout} rope={rope}: max |got - exact| / (2^-20 (|y_2i| + |y_2i+1|)) = {worst:.3f}")


def test_head_post_f32_refuses_what_it_cannot_address(dev):
    from actionmesh_amd import ops
    x = torch.zeros((4, 3 * HD), device=dev)
    w = torch.ones((HD,), device=dev)
    with pytest.raises(ValueError, match="columns"):
        ops.head_post_f32(x, 2, w, off=0, head_stride=3 * HD)             # head 1 would end at column 4 hd
    with pytest.raises(RuntimeError, match="overlap"):
        ops.head_post_f32(x, 2, w, off=0, head_stride=64)                 # in place: overlapping chunks are refused by the library
    cos = torch.ones((1, HD // 2), device=dev)
    with pytest.raises(ValueError, match="frames"):
        ops.head_post_f32(x, 1, w, rope=(cos, cos), rows_per_frame=3)     # row 3 is frame 1, the tables hold one


def test_head_post_f32_rotation_is_rope_f32_bit_for_bit(dev):
    """The two kernels share one rotation: am_head_post_f32 with tables on the q chunks gives, bit for bit, am_head_post_f32 without
    tables followed by am_rope_f32 (one kind) on the same chunks - the file is built without contraction, and the store and reload of
    the normalised fp32 values between the two launches keeps their bits.  The packed [q | k | v] layout: 11 rows of 3 heads, head
    stride 3 x 128, 4 rows per frame (three frames, the last partial), a row stride 4 floats wider than the row; 33 chunks over five
    8-chunk workgroups, the last one partial.  X sits in a poisoned arena, the gain and the tables in arenas of their own, the values
    are finite; the k and v chunks and the gap keep their bits."""
    from actionmesh_amd import ops
    from actionmesh_amd.denoiser import rope_tables_host
    gen = torch.Generator().manual_seed(23)
    rows, heads, hs, rpf = 11, 3, 3 * HD, 4
    width = hs * heads
    x = torch.randn((rows, width), generator=gen) * 3.0
    w = 1.0 + 0.1 * torch.randn((HD,), generator=gen)
    cos, sin = rope_tables_host(torch.arange(3, dtype=torch.float32)[None] * 1.5 + 2.0)
    Wt, Cs, Sn = (Arena.flat_of(t.to(dev)) for t in (w, cos, sin))
    tabs = (Cs.view, Sn.view)
    fused, split = Arena.of(x.to(dev), ld=width + 4), Arena.of(x.to(dev), ld=width + 4)
    ops.head_post_f32(fused.view, heads, Wt.view, off=0, head_stride=hs, rope=tabs, rows_per_frame=rpf)
    ops.head_post_f32(split.view, heads, Wt.view, off=0, head_stride=hs)
    normed = split.view.cpu()
    ops.rope_f32(split.view, heads, tabs, off_a=0, off_b=-1, head_stride=hs, rows_per_frame=rpf)
    torch.cuda.synchronize()
    for a, what in ((fused, "X, one launch"), (split, "X, two launches"), (Wt, "w"), (Cs, "cos"), (Sn, "sin")):
        a.assert_untouched(what)
    assert torch.equal(Wt.view.cpu(), w) and torch.equal(Cs.view.cpu(), cos) and torch.equal(Sn.view.cpu(), sin)
    got, two = fused.view.cpu(), split.view.cpu()
    assert torch.isfinite(got).all()
    assert torch.equal(got.view(torch.int32), two.view(torch.int32)), f"{int((got != two).sum())} element(s) differ"
    q = torch.zeros((rows, width), dtype=torch.bool)
    for h in range(heads):
        q[:, h * hs: h * hs + HD] = True
    assert torch.equal(got[~q].view(torch.int32), x[~q].view(torch.int32)), "a k or v chunk changed"
    assert not torch.equal(got[q], normed[q]) and not torch.equal(normed[q], x[q])          # both steps did something


# ---- am_flow_step_f32 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("additive", [True, False])
@pytest.mark.parametrize("nb", [1, 2, 3])
@pytest.mark.parametrize("N,D", [(7, 12), (7, 13)])
def test_flow_step_f32_is_the_torch_fp32_expression(dev, N, D, nb, additive):
    """Bit-identical to O.aggregate_cfg / O.flow_sample's fp32 step: 1, 2 and 3 branches, additive and subtractive, observed frames at
    both ends of the mask, on frames 1 .. 4 of six (the frames in front and behind are guards of their own), latents and velocity in
    guard-band arenas.  N x D = 84 takes the 16-byte path, 91 (no multiple of 4) the element path."""
    from actionmesh_amd import ops
    from oracle import denoiser_oracle as O
    gen = torch.Generator().manual_seed(11 + nb)
    T, scales, dt = 4, [7.5, 1.3][:nb - 1], 0.0356
    unobserved = [False, True, True, False]
    v = torch.randn((nb, T, N, D), generator=gen)
    lat = torch.randn((T + 2, N, D), generator=gen)
    out = O.aggregate_cfg(v, nb, scales, O.Precision("fp32"))[0]
    step = torch.tensor(dt, dtype=torch.float32) * out
    flow = lat[1:5] + step if additive else lat[1:5] - step
    want = lat.clone()
    want[1:5][torch.tensor(unobserved)] = flow[torch.tensor(unobserved)]
    V = Arena.flat_of(v.to(dev))
    Lt = Arena.flat_of(lat.to(dev))
    ops.flow_step(V.view, Lt.view[1:5], scales, dt, additive, unobserved)          # dispatches on the velocity's dtype
    torch.cuda.synchronize()
    V.assert_untouched("v"); Lt.assert_untouched("latents")
    assert torch.equal(V.view.cpu(), v)
    got = Lt.view.cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), float((got - want).abs().max())
    assert torch.equal(got[[0, 1, 4, 5]], lat[[0, 1, 4, 5]]) and not torch.equal(got[2:4], lat[2:4])
    plain = lat[1:5].clone().to(dev)
    ops.flow_step_f32(v.to(dev), plain, scales, dt, additive, None)                 # no mask: every frame
    assert torch.equal(plain.cpu().view(torch.int32), flow.view(torch.int32))


# ---- HipDenoiser(dtype="float32") on the tiny fixtures: the CPU file's assertions on the kernels ----------------------------------
@pytest.mark.parametrize("name", list(S.CASES))
def test_forward_against_the_reference_fp32_velocity(dev, golden_dir, name):
    """seen: tiny_inflated 7.75e-7, tiny_mixed 7.71e-7"""
    model, _ = S.check_forward(name, golden_dir, dev)
    # three forwards: the first binds, the second reuses the cache, the third re-binds for the other context tensor
    e = model._engine
    counts = e.entry_counts()
    NL, n_skip = e.NL, sum(1 for i in range(e.NL) if e.has_skip(i))
    assert e.kind == "f32" and set(counts) == S.F32_ENTRIES - {"am_flow_step_f32"}, counts
    assert counts["am_attention_f32"] == 3 * 2 * NL and counts["am_head_post_f32"] == 3 * 3 * NL + 2 * NL
    assert counts["am_gemm_f32"] == 3 * (4 + 6 * NL + 2 * n_skip) + 2 * NL
    assert not hasattr(e, "handle")                          # no am_handle: the 16-bit engine's C forward cannot have run


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("name", list(S.CASES))
def test_sampler_loop_against_the_reference_fp32_latents(dev, golden_dir, name, split):
    """seen: tiny_inflated 3.7e-7 after step 1 growing to 1.32e-6 after step 4, tiny_mixed 4.8e-7 to 1.74e-6 after step 3; the
    split_cfg_batch runs give the same figures, final against the reference's split run 1.32e-6 / 1.74e-6"""
    model, curve, final = S.check_loop(name, golden_dir, dev, split=split)
    assert set(model._engine.entry_counts()) <= S.F32_ENTRIES and model._engine.kind == "f32"


def test_autocast_region_changes_nothing(dev, golden_dir):
    """The reference pipeline runs Stage I inside torch.autocast("cuda", dtype) (pipeline.py:671): a 16-bit model takes its type from
    the region, the fp32 model computes the same bits inside it as outside."""
    g, model, t = S.setup("tiny_mixed", golden_dir, dev)
    x_in, c_in, m_in, f_in = (a.to(dev) for a in S.guidance().cfg_at_inference(t["init_latent"], t["context"], t["mask"], t["framestep"]))
    tt = torch.tensor([float(g["fwd_t"])]).expand(2).to(dev)
    v, _ = model.forward(x_in, c_in, f_in, tt, m_in, None)
    with torch.autocast("cuda", dtype=torch.float16):
        assert model.compute_kind() == "f32"
        va, _ = model.forward(x_in, c_in, f_in, tt, m_in, None)
    assert va.dtype == torch.float32 and torch.equal(va, v)


def test_both_library_builds_give_the_same_bits(dev):
    """The new entry points are in libactionmesh_amd.so and in the float16 build, the same object code."""
    from actionmesh_amd import ops
    from actionmesh_amd.denoiser import rope_tables_host
    gen = torch.Generator().manual_seed(3)
    x = torch.randn((10, 3 * HD * 2), generator=gen).to(dev)
    w = (1.0 + 0.1 * torch.randn((HD,), generator=gen)).to(dev)
    cos, sin = (t.to(dev) for t in rope_tables_host(torch.arange(2, dtype=torch.float32)[None]))
    a = ops.head_post_f32(x.clone(), 2, w, off=HD, head_stride=3 * HD, rope=(cos, sin), rows_per_frame=5, kind="bf16")
    b = ops.head_post_f32(x.clone(), 2, w, off=HD, head_stride=3 * HD, rope=(cos, sin), rows_per_frame=5, kind="f16")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and not torch.equal(a, x)
    v = torch.randn((2, 3, 5, 8), generator=gen).to(dev)
    la, lb = torch.zeros((3, 5, 8), device=dev), torch.zeros((3, 5, 8), device=dev)
    ops.flow_step_f32(v, la, [7.5], 0.1, True, None, kind="bf16")
    ops.flow_step_f32(v, lb, [7.5], 0.1, True, None, kind="f16")
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32)) and bool(la.ne(0).any())


# ---- the headline architecture: 21 layers, skip depth 10, width 1024, T = 8, N = 256, S = 257 ---------------------------------------
@pytest.fixture(scope="module")
def headline(dev, golden_dir):
    """arch_headline's weights and inputs (regenerated from seeds and pinned by the fixture's checksums), the fp32 model and its one
    forward at the fixture's time: computed once, shared by the tests below."""
    from actionmesh_amd import HipDenoiser
    from oracle.denoiser_oracle import state_dict_checksum
    from oracle.make_golden_baseline import baseline_case_inputs, tensor_checksum
    g = np.load(os.path.join(golden_dir, "arch_headline.npz"))
    kw, cfg, sd, inp, steps = baseline_case_inputs("arch_headline")
    assert state_dict_checksum(sd) == pytest.approx(float(g["weights_checksum"]), rel=1e-12)
    assert np.allclose([tensor_checksum(inp[k]) for k in ("init_latent", "context", "mask", "framestep")], g["inputs_checksum"], rtol=1e-12)
    T, N = inp["init_latent"].shape[1:3]

    def build(**model_kw):
        m = HipDenoiser(num_tokens_nominal=N, temporal_context_size=T, **kw, **model_kw)
        m.load_state_dict(sd)
        return m.to(dev).eval()

    def forward(m):
        x_in, c_in, m_in, f_in = S.guidance().cfg_at_inference(inp["init_latent"], inp["context"], inp["mask"], inp["framestep"])
        tt = torch.tensor([float(g["fwd_t"])]).expand(2)
        v, _ = m.forward(x_in.to(dev), c_in.to(dev), f_in.to(dev), tt.to(dev), m_in.to(dev), None)
        torch.cuda.synchronize()
        return v.float().cpu()
    model = build(dtype="float32")
    return dict(g=g, inp=inp, steps=steps, model=model, v32=forward(model), build=build, forward=forward)


def test_headline_forward_against_the_reference_fp32_velocity(headline):
    """seen: 1.57e-6"""
    r = S.rel(headline["v32"], torch.from_numpy(headline["g"]["fwd_velocity_fp32"]))
    print(f"arch_headline: device fp32 forward rel-L2 vs the reference's fp32 velocity {r:.3e}")
    assert r <= S.BOUND, r


def test_headline_sampler_loop_against_the_reference_fp32_latents(dev, headline):
    """30 steps; at every step rel-L2 on the stored token subset <= max(2e-5, ref_autocast_curve[step] / 100), and the full final latents
    against loop_final_fp32 under the last step's bound.
    seen: 1.02e-7 after step 1 growing to 1.57e-6 after step 30 (bounds 2e-5 .. 1.40e-4); final full latents 1.57e-6"""
    from actionmesh_amd import HipSchedulerFlow
    g, inp, steps, model = headline["g"], headline["inp"], headline["steps"], headline["model"]
    stride = int(g["token_stride"])
    ref, ref_curve = torch.from_numpy(g["loop_latents_sub_fp32"]), g["ref_autocast_curve"]
    assert steps == 30 and len(ref_curve) == steps
    sched = HipSchedulerFlow(num_inference_steps=steps, shift=3.0, is_additive=True)
    curve, last = [], None
    for i, (lat, _t) in enumerate(sched._flow_sample(model, S.guidance(), inp["init_latent"].clone().to(dev), inp["context"].to(dev),
                                                     device=dev, mask=inp["mask"].to(dev), framestep=inp["framestep"].to(dev))):
        sub = lat[:, :, ::stride].cpu()
        assert torch.equal(sub[0, 0], inp["init_latent"][0, 0, ::stride]), "conditioning frame must stay untouched"
        curve.append(S.rel(sub, ref[i]))
        last = lat
    bounds = [max(S.BOUND, float(c) / 100) for c in ref_curve]
    final = S.rel(last.cpu(), torch.from_numpy(g["loop_final_fp32"]))
    print("arch_headline: device fp32 per-step latents rel-L2 vs the reference's fp32 loop: " + " ".join(f"{c:.2e}" for c in curve))
    print("arch_headline: bound max(2e-5, ref_autocast_curve / 100):                        " + " ".join(f"{b:.2e}" for b in bounds))
    print(f"arch_headline: device fp32 final full latents rel-L2 {final:.3e}")
    assert len(curve) == steps
    for i, c in enumerate(curve):
        assert c <= bounds[i], (i, c, bounds[i])
    assert final <= bounds[-1], (final, bounds[-1])
    assert set(model._engine.entry_counts()) <= S.F32_ENTRIES


def test_device_fp32_stands_in_for_the_host_fp32_forward(headline):
    """The yardstick in use: the bf16 model's one-forward distance to the DEVICE fp32 run and to the fixture's fp32 velocity (a host forward
    of the reference's own modules) agree within 2 % of each other.
    seen: 9.7826e-3 vs 9.7826e-3 (relative difference 4.0e-8)"""
    bf16 = headline["build"]()
    vb = headline["forward"](bf16)
    bf16.cpu()
    assert bf16.compute_kind() == "bf16" and vb.shape == headline["v32"].shape
    r_dev = S.rel(vb, headline["v32"])
    r_fix = S.rel(vb, torch.from_numpy(headline["g"]["fwd_velocity_fp32"]))
    print(f"arch_headline: bf16 forward rel-L2 vs the device fp32 run {r_dev:.4e}, vs the reference's fp32 velocity {r_fix:.4e} "
          f"(relative difference {abs(r_dev - r_fix) / r_fix:.2e})")
    assert abs(r_dev - r_fix) <= 0.02 * r_fix, (r_dev, r_fix)
