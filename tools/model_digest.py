#!/usr/bin/env python3
"""Digests of the Stage-I forward, for comparing two builds of the library entry for entry.

Builds seeded models through HipEngine (weights: oracle.denoiser_oracle.synthetic_state_dict) and prints one JSON line: for every
selected (model, mode) the sha256 of the output velocity bytes of an untraced forward, and for model A the (tag, checksum) list of a
forward under am_debug_trace_begin / _end as well.

  model A   tiny_mixed (tests/test_denoiser_gpu.py): 5 layers, skips on 3 and 4, per-frame layer 2; B=2 T=4 N=48 S=20
            modes 1 default, 2 branch hints, 3 ACTIONMESH_AMD_LN_FOLD=0, 4 ACTIONMESH_AMD_LN_STATS=recompute, 5 fp8, 6 fp8_fast,
            7 am_denoise_forward_graph three times (eager, capture, replay)
  model A2  three inflated layers, B=2 T=8 N=511, two engines on one device on the two-pass overlap path: modes 1 bf16, 2 fp8
  model B   width 1024, 8 heads, 3 layers (0 and 2 inflated, skip on 2), B=2 T=6 N=1024 (M = 12300 rows): modes 1 default, 2 hints

--time LEGS (with one model and one mode) prints the median host time of an eager forward instead: wall clock around a
synchronisation, --forwards forwards per leg.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from actionmesh_amd import _lib as L                                                  # noqa: E402
from actionmesh_amd.denoiser import HipEngine, rope_tables_host                      # noqa: E402
from actionmesh_amd.sharding import FrameShardPlan                                    # noqa: E402
from oracle import denoiser_oracle as O                                               # noqa: E402

MODELS = {
    "A": (dict(in_channels=64, num_layers=5, num_attention_heads=2, width=256, mlp_ratio=4.0, cross_attention_dim=64,
               inflated_layers=(0, 1, 3, 4)), (2, 4, 48, 20), 0, (1, 2, 3, 4, 5, 6, 7)),
    "A2": (dict(in_channels=64, num_layers=3, num_attention_heads=2, width=256, mlp_ratio=4.0, cross_attention_dim=64,
                inflated_layers=(0, 1, 2)), (2, 8, 511, 9), 3, (1, 2)),
    "B": (dict(in_channels=64, num_layers=3, num_attention_heads=8, width=1024, mlp_ratio=4.0, cross_attention_dim=256,
               inflated_layers=(0, 2)), (2, 6, 1024, 20), 0, (1, 2)),
}
ENV = {3: ("ACTIONMESH_AMD_LN_FOLD", "0"), 4: ("ACTIONMESH_AMD_LN_STATS", "recompute")}


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def inputs(hp, shape, hints):
    B, T, N, S = shape
    g = torch.Generator().manual_seed(11)
    x = torch.randn((B, T, N, hp["in_channels"]), generator=g)
    ctx = torch.randn((B, T, S, hp["cross_attention_dim"]), generator=g)
    if hints:                       # what the hints state: row 0's context is zero, all rows share hidden_states and times
        x[1:] = x[0]
        ctx[0] = 0
    cos, sin = rope_tables_host(torch.arange(T).repeat(B, 1), 128)
    return x, ctx, [0.37] * (B * T), cos, sin


def traced(lib, dev, fwd):
    klog = torch.zeros(4096, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    L.check(lib.am_debug_trace_begin(klog.data_ptr(), klog.numel()), "am_debug_trace_begin")
    try:
        fwd()
    finally:
        tags = (C.c_int32 * 4096)(); n = C.c_int()
        L.check(lib.am_debug_trace_end(tags, 4096, C.byref(n)), "am_debug_trace_end")
    torch.cuda.synchronize()
    return [[t, f"{c & 0xFFFFFFFFFFFFFFFF:016x}"] for t, c in zip(list(tags)[:n.value], klog[:n.value].cpu().tolist())]


def single(name, mode, dev, forwards, legs):
    hp, shape, seed, _ = MODELS[name]
    B, T, N, S = shape
    sd = O.synthetic_state_dict(O.OracleConfig(**hp), seed=seed)
    x, ctx, t_bt, cos, sin = inputs(hp, shape, hints=mode == 2)
    if mode in ENV:                 # read by am_create
        os.environ[ENV[mode][0]] = ENV[mode][1]
    try:
        e = HipEngine(hp, sd, dev, B, T, N, S, attn_dtype={5: "fp8", 6: "fp8_fast"}.get(mode, "bf16"), use_graph=mode == 7)
    finally:
        if mode in ENV:
            del os.environ[ENV[mode][0]]
    e.set_context(ctx.to(dev), cos, sin, ctx_zero=[True, False] if mode == 2 else None, shared_prefix=mode == 2)
    xd = x.to(dev)
    out = {}
    if legs:
        e.forward(xd, t_bt); torch.cuda.synchronize()
        meds = []
        for _ in range(legs):
            ts = []
            for _ in range(forwards):
                t0 = time.perf_counter()
                e.forward(xd, t_bt); torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            meds.append(statistics.median(ts) * 1e6)
        out["host_us_leg_medians"] = meds
    elif mode == 7:
        out["velocity_sha256"] = [sha(e.forward(xd, t_bt)) for _ in range(3)]
        out["graph_stats"] = list(e.graph_stats())
        assert out["graph_stats"] == [1, 1, 1, 0], out["graph_stats"]
    else:
        out["velocity_sha256"] = [sha(e.forward(xd, t_bt)) for _ in range(forwards)][-1]
        if name == "A":
            out["trace"] = traced(e.lib, dev, lambda: e.forward(xd, t_bt))
    e.close()
    return out


def overlap(mode, dev):
    """Two ranks of a world of 2 on one device, the all-gather done by hand between the local pass and the resume pass."""
    hp, shape, seed, _ = MODELS["A2"]
    B, T, N, S = shape
    sd = O.synthetic_state_dict(O.OracleConfig(**hp), seed=seed)
    x, ctx, t_bt, cos, sin = inputs(hp, shape, hints=False)
    engines = []
    for r in range(2):
        plan = FrameShardPlan(T, 2, r)
        e = HipEngine(hp, sd, dev, B, plan.frames_local, N, S, world=2, rank=r, attn_dtype="fp8" if mode == 2 else "bf16")
        e.set_context(plan.slice_frames(ctx.to(dev)), cos.view(B, T, -1)[:, plan.frame_slice].reshape(-1, 64),
                      sin.view(B, T, -1)[:, plan.frame_slice].reshape(-1, 64))
        tl = plan.frames_local
        e.begin(plan.slice_frames(x.to(dev)), [t_bt[b * T + r * tl + j] for b in range(B) for j in range(tl)])
        engines.append(e)
    for i in range(hp["num_layers"]):
        for e in engines:
            e.layer_pre(i)
        for e in engines:
            e.layer_attn_local(i)
        bufs = [e.kv_buffers()[0] for e in engines]
        assert all((b.dtype == torch.uint8) == (mode == 2) for b in bufs)
        for r, dst in enumerate(bufs):
            for s_, src in enumerate(bufs):
                if s_ != r:
                    dst[s_].copy_(src[s_])
        for e in engines:
            e.layer_post(i)
    out = {"velocity_sha256": sha(torch.cat([e.end() for e in engines], dim=1)),
           "attention_counters": [list(e.attention_counters()) for e in engines]}
    for e in engines:
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="all", choices=["all"] + list(MODELS))
    ap.add_argument("--mode", type=int, default=0, help="0: every mode of the model")
    ap.add_argument("--forwards", type=int, default=1)
    ap.add_argument("--time", type=int, default=0, metavar="LEGS")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "model_digest.py needs a GPU"
    dev = torch.device("cuda:0")
    res = {}
    for name in (MODELS if a.model == "all" else [a.model]):
        for mode in MODELS[name][3]:
            if a.mode in (0, mode):
                res[f"{name}.{mode}"] = overlap(mode, dev) if name == "A2" else single(name, mode, dev, a.forwards, a.time)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
