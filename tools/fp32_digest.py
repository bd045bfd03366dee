#!/usr/bin/env python3
"""Digests of the exact-fp32 path, for comparing two commits bit for bit.

Prints one JSON line of sha256 digests of output bytes on seeded inputs, through the surface every commit with the exact-fp32 path
has (ops.*_f32, HipDenoiser, HipAutoencoder, HipImageEncoder, HipSchedulerFlow), so the same file runs from either checkout (the
libraries: ACTIONMESH_AMD_LIB / ACTIONMESH_AMD_LIB_F16, or the checkout's own).

  kernels  head_post_f32 with and without tables; rope_f32 with one and two kinds; flow_step_f32 with 1, 2 and 3 branches on a frame
           size that takes the 16-byte path (84) and one that takes the element path (91), masked and unmasked; attention_f32 in the
           packed [q | k | v] and the [k | v] layouts at sq = 33, sk = 65
  models   Stage I tiny_mixed: one forward and a 2-step sampler loop; Stage II ae_tiny: exact_fp32, and cross_fp32 under bfloat16 and
           float16; the image encoder in float32 at head_dim 64 (28 x 42 pixels) and 128 (42 x 28)
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from actionmesh_amd import ClassifierFreeGuidance, HipAutoencoder, HipDenoiser, HipImageEncoder, HipSchedulerFlow, ops   # noqa: E402
from actionmesh_amd.denoiser import rope_tables_host                                                                      # noqa: E402
from oracle import autoencoder_oracle as AO                                                                               # noqa: E402
from oracle import denoiser_oracle as O                                                                                   # noqa: E402
from oracle import dinov2_oracle as DO                                                                                    # noqa: E402

HD = 128
GOLDEN = os.path.join(ROOT, "tests", "golden")


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def kernels(dev):
    res = {}
    gen = torch.Generator().manual_seed(5)
    rows, heads, hs, rpf = 11, 3, 3 * HD, 4
    x = (torch.randn((rows, hs * heads), generator=gen) * 3.0).to(dev)
    w = (1.0 + 0.1 * torch.randn((HD,), generator=gen)).to(dev)
    tabs = tuple(t.to(dev) for t in rope_tables_host(torch.arange(3, dtype=torch.float32)[None] * 1.5 + 2.0))
    res["head_post_f32.tables"] = sha(ops.head_post_f32(x.clone(), heads, w, off=HD, head_stride=hs, rope=tabs, rows_per_frame=rpf))
    res["head_post_f32.plain"] = sha(ops.head_post_f32(x.clone(), heads, w, off=0, head_stride=hs))
    res["rope_f32.one_kind"] = sha(ops.rope_f32(x.clone(), heads, tabs, off_a=HD, off_b=-1, head_stride=hs, rows_per_frame=rpf))
    res["rope_f32.two_kinds"] = sha(ops.rope_f32(x.clone(), heads, tabs, off_a=0, off_b=HD, head_stride=hs, rows_per_frame=rpf))
    for N, D in ((7, 12), (7, 13)):                                   # N D = 84: the 16-byte path; 91: the element path
        for nb in (1, 2, 3):
            v = torch.randn((nb, 4, N, D), generator=gen).to(dev)
            lat = torch.randn((4, N, D), generator=gen).to(dev)
            for mask in (None, [False, True, True, False]):
                out = lat.clone()
                ops.flow_step_f32(v, out, [7.5, 1.3][:nb - 1], 0.0356, nb != 2, mask)
                res[f"flow_step_f32.{N * D}.nb{nb}.{'masked' if mask else 'all'}"] = sha(out)
    nseq, H, sq, sk = 2, 3, 33, 65
    for s in (sq, sk):                                                # one packed tensor: as many queries as keys
        qkv = torch.randn((nseq * s, 3 * HD * H), generator=gen).to(dev)
        res[f"attention_f32.packed_qkv.s{s}"] = sha(ops.attention_f32(qkv, qkv, qkv, H, s, s, HD, q_hs=3 * HD, k_hs=3 * HD, v_hs=3 * HD,
                                                                      q_off=0, k_off=HD, v_off=2 * HD))
    for D in (64, 128):
        q = torch.randn((nseq * sq, H * D), generator=gen).to(dev)
        kv = torch.randn((nseq * sk, 2 * H * D), generator=gen).to(dev)
        res[f"attention_f32.kv.d{D}"] = sha(ops.attention_f32(q, kv, kv, H, sq, sk, D, q_hs=D, k_hs=2 * D, v_hs=2 * D, v_off=D))
    return res


def stage1(dev):
    hp = dict(in_channels=64, num_layers=5, num_attention_heads=2, width=256, mlp_ratio=4.0, cross_attention_dim=64,
              inflated_layers=(0, 1, 3, 4))
    g = np.load(os.path.join(GOLDEN, "tiny_mixed.npz"))
    model = HipDenoiser(num_tokens_nominal=48, temporal_context_size=4, dtype="float32", **hp)
    model.load_state_dict(O.synthetic_state_dict(O.OracleConfig(**hp), seed=0))
    model.to(dev).eval()
    t = {k: torch.from_numpy(g[k]).to(dev) for k in ("init_latent", "context", "mask", "framestep")}
    cfg = ClassifierFreeGuidance(True, [[0, 1], [1, 1]], [7.5])
    x_in, c_in, m_in, f_in = cfg.cfg_at_inference(t["init_latent"], t["context"], t["mask"], t["framestep"])
    tt = torch.tensor([float(g["fwd_t"])]).expand(2).to(dev)
    v, _ = model.forward(x_in, c_in, f_in, tt, m_in, None)
    res = {"stage1.tiny_mixed.forward": sha(v)}
    sched = HipSchedulerFlow(num_inference_steps=2, shift=3.0, is_additive=True)
    for i, (lat, _t) in enumerate(sched._flow_sample(model, cfg, t["init_latent"].clone(), t["context"], device=dev, mask=t["mask"],
                                                     framestep=t["framestep"])):
        res[f"stage1.tiny_mixed.loop_step{i + 1}"] = sha(lat)
    return res


def stage2(dev):
    g = np.load(os.path.join(GOLDEN, "ae_tiny.npz"))
    width, layers, heads, latent = (int(v) for v in g["config"])
    cfg = AO.AEConfig(width=width, num_layers=layers, num_attention_heads=heads, latent_channels=latent)
    sd = AO.synthetic_state_dict(cfg, seed=0)
    t = {k: torch.from_numpy(g[k]) for k in ("latent", "framestep", "source_alpha", "target_alphas", "query")}
    res = {}
    for name, kw, dtype in (("exact_fp32", dict(exact_fp32=True), None), ("cross_fp32.bf16", dict(cross_fp32=True), torch.bfloat16),
                            ("cross_fp32.f16", dict(cross_fp32=True), torch.float16)):
        m = HipAutoencoder(in_extra_channels=cfg.in_extra_channels, width=width, num_layers=layers, num_attention_heads=heads,
                           latent_channels=latent, embed_include_pi=cfg.embed_include_pi, **kw)
        m.load_state_dict(sd)
        m.to(dev).eval()
        with torch.autocast("cuda", dtype=dtype, enabled=dtype is not None):
            d = m(t["latent"].to(dev), t["framestep"], t["source_alpha"], t["target_alphas"], t["query"].to(dev))
        res[f"stage2.ae_tiny.{name}"] = sha(d)
    return res


def encoder(dev):
    res = {}
    for C, height, width in ((128, 28, 42), (256, 42, 28)):
        cfg = DO.DinoConfig(hidden_size=C, num_hidden_layers=2, num_attention_heads=2)
        enc = HipImageEncoder(config=vars(cfg), state_dict=DO.synthetic_state_dict(cfg, seed=3), dtype="float32").to(dev)
        pixels = torch.randn((2, 3, height, width), generator=torch.Generator().manual_seed(C + height))
        res[f"encoder.float32.head_dim_{C // 2}"] = sha(enc.encode_pixels(pixels.to(dev)))
    return res


def main():
    assert torch.cuda.is_available(), "fp32_digest.py needs a GPU"
    dev = torch.device("cuda:0")
    res = {}
    for part in (kernels, stage1, stage2, encoder):
        res.update(part(dev))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
