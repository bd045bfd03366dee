"""How far are the 16-bit and fp8 Stage-I modes from fp32 - measured against the DEVICE fp32 run, HipDenoiser(dtype="float32").

One process, one device.  Per case the fp32 model and the 16-bit model(s) are built from the same weights and inputs:
  * a fixture name (`--case arch_headline`, `--case full_headline`, ...): the seeded weights and inputs of
    oracle.make_golden_baseline.baseline_case_inputs, the ones tests/golden/<name>.npz was computed from;
  * or a checkpoint directory (`--weights DIR`, read with from_pretrained: config.json + model.safetensors) with seeded inputs of
    `--frames` x `--tokens` latent tokens and `--ctx-tokens` context tokens - a user's own check of their own weights.
Reported per case, as one JSON document (`--out`, and stdout):
  (a) rel-L2 of each mode of `--modes` (bf16, float16, fp8, fp8_fast) against the device fp32 run: one forward (both CFG branches, the
      fixture's diffusion time), and the latents after every step of a `--steps N` sampler loop;
  (b) where the fixture exists: the device fp32 forward against the reference's own fp32 velocity (for full_headline / full_nominal the
      every-64th-token subset the fixture keeps - the two checks too long for the test suite), and the fp32 loop against the
      fixture's per-step latents as far as both go;
  (c) the fp32 forward's wall time around a device synchronisation, median of 3 after one warm-up forward, with the algorithmic
      work (oracle.step_flops) beside it.

    python tools/stage1_fp32_probe.py --case full_headline:3 --case full_nominal:3 --case arch_headline:30 --case arch_headline_peaky:10
                                        --out profiles/stage1_fp32.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from actionmesh_amd import ClassifierFreeGuidance, HipDenoiser, HipSchedulerFlow  # noqa: E402
from oracle import denoiser_oracle as O  # noqa: E402

MODES = {"bf16": {}, "float16": {"dtype": "float16"}, "fp8": {"attn_dtype": "fp8"}, "fp8_fast": {"attn_dtype": "fp8_fast"}}
GUIDANCE, SCALES, FWD_T = [[0, 1], [1, 1]], [7.5], 700.0


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def fixture_case(name):
    """(make(**kw) -> HipDenoiser on the CPU, inputs, OracleConfig, fixture or None)"""
    from oracle.make_golden_baseline import baseline_case_inputs
    kw, cfg, sd, inp, _ = baseline_case_inputs(name)
    T, N = inp["init_latent"].shape[1:3]

    def make(**model_kw):
        m = HipDenoiser(num_tokens_nominal=N, temporal_context_size=T, **kw, **model_kw)
        m.load_state_dict(sd)
        return m
    path = os.path.join(ROOT, "tests", "golden", f"{name}.npz")
    return make, inp, cfg, (np.load(path) if os.path.exists(path) else None)


def checkpoint_case(path, T, N, S, seed):
    probe = HipDenoiser.from_pretrained(path)
    cfg = O.OracleConfig(**probe.hyper_params())
    sd = probe._host_sd

    def make(**model_kw):
        m = HipDenoiser(num_tokens_nominal=probe.num_tokens_nominal, temporal_context_size=probe.temporal_context_size,
                        **probe.hyper_params(), **model_kw)
        m.load_state_dict(sd)
        return m
    g = torch.Generator().manual_seed(seed)
    mask = torch.zeros(1, T)
    mask[0, 0] = 1.0                                   # frame 0 is the conditioning frame
    inp = dict(init_latent=torch.randn(1, T, N, cfg.in_channels, generator=g), context=torch.randn(1, T, S, cfg.cross_attention_dim, generator=g),
               mask=mask, framestep=torch.arange(T, dtype=torch.float32)[None])
    return make, inp, cfg, None


def forward(model, inp, dev, t=FWD_T):
    """One forward of both CFG branches; (velocity on the CPU as fp32, seconds around a synchronise)."""
    cfgd = ClassifierFreeGuidance(True, GUIDANCE, SCALES)
    x_in, c_in, m_in, f_in = (a.to(dev) for a in cfgd.cfg_at_inference(inp["init_latent"], inp["context"], inp["mask"], inp["framestep"]))
    tt = torch.tensor([t]).expand(len(GUIDANCE)).to(dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    v, _ = model.forward(x_in, c_in, f_in, tt, m_in, None)
    torch.cuda.synchronize(dev)
    return v.float().cpu(), time.perf_counter() - t0


def loop(model, inp, dev, steps):
    """The latents after every step of a `steps`-step sampler loop (CPU, fp32)."""
    sched = HipSchedulerFlow(num_inference_steps=steps, shift=3.0, is_additive=True)
    cfgd = ClassifierFreeGuidance(True, GUIDANCE, SCALES)
    out = []
    for lat, _t in sched._flow_sample(model, cfgd, inp["init_latent"].clone().to(dev), inp["context"].to(dev), device=dev,
                                      mask=inp["mask"].to(dev), framestep=inp["framestep"].to(dev)):
        out.append(lat.float().cpu().clone())
    return out


def probe(label, case, modes, steps, dev):
    make, inp, cfg, g = case
    _, T, N, _ = inp["init_latent"].shape
    S = inp["context"].shape[2]
    rec = dict(case=label, frames=T, tokens=N, ctx_tokens=S, width=cfg.width, layers=cfg.num_layers, branches=len(GUIDANCE), steps=steps,
               forward_flops=O.step_flops(len(GUIDANCE), T, N, cfg, S))
    m32 = make(dtype="float32").to(dev).eval()
    v32, warm = forward(m32, inp, dev)
    times = [forward(m32, inp, dev)[1] for _ in range(3)]
    rec["fp32_forward_seconds"] = dict(median_of_3=statistics.median(times), all=times, first=warm)
    rec["fp32_forward_tflops"] = rec["forward_flops"] / statistics.median(times) / 1e12
    print(f"[{label}] fp32 forward {statistics.median(times):.3f} s (first {warm:.3f} s), {rec['fp32_forward_tflops']:.1f} TFLOP/s algorithmic", flush=True)
    if g is not None:                                                                     # (b)
        if "fwd_velocity_fp32" in g.files:
            rec["fp32_forward_vs_reference_fp32"] = rel(v32, torch.from_numpy(g["fwd_velocity_fp32"]))
        elif "fwd_velocity_fp32_sub" in g.files:
            stride = int(g["token_stride"])
            rec["fp32_forward_vs_reference_fp32"] = rel(v32[:, :, ::stride], torch.from_numpy(g["fwd_velocity_fp32_sub"]))
            rec["reference_token_stride"] = stride
        if "fwd_ref_autocast_vs_fp32" in g.files:
            rec["reference_autocast_bf16_vs_its_fp32"] = float(g["fwd_ref_autocast_vs_fp32"])
        print(f"[{label}] device fp32 forward vs the reference's fp32 velocity: {rec.get('fp32_forward_vs_reference_fp32')}", flush=True)
    lat32 = loop(m32, inp, dev, steps) if steps else []
    if g is not None and steps and "loop_latents_sub_fp32" in g.files and int(g["steps"]) == steps:
        stride, ref = int(g["token_stride"]), torch.from_numpy(g["loop_latents_sub_fp32"])
        rec["fp32_loop_vs_reference_fp32"] = [rel(lat32[i][:, :, ::stride], ref[i]) for i in range(steps)]
    m32.cpu()                                                                             # frees the engine: weights, K / V
    del m32
    rec["modes"] = {}
    for mode in modes:                                                                    # (a)
        m = make(**MODES[mode]).to(dev).eval()
        v, _ = forward(m, inp, dev)
        r = dict(forward_vs_device_fp32=rel(v, v32))
        if g is not None and "fwd_velocity_fp32" in g.files:
            r["forward_vs_reference_fp32"] = rel(v, torch.from_numpy(g["fwd_velocity_fp32"]))
        elif g is not None and "fwd_velocity_fp32_sub" in g.files:
            r["forward_vs_reference_fp32"] = rel(v[:, :, ::int(g["token_stride"])], torch.from_numpy(g["fwd_velocity_fp32_sub"]))
        if steps:
            r["loop_vs_device_fp32"] = [rel(a, b) for a, b in zip(loop(m, inp, dev, steps), lat32)]
        m.cpu()
        del m
        rec["modes"][mode] = r
        print(f"[{label}] {mode}: forward vs device fp32 {r['forward_vs_device_fp32']:.4e}"
              + (f", after step {steps}: {r['loop_vs_device_fp32'][-1]:.4e}" if steps else ""), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--case", action="append", default=[], metavar="NAME[:STEPS]",
                    help="a fixture name of oracle/make_golden_baseline.py, optionally with its own number of sampler steps (repeatable)")
    ap.add_argument("--weights", default=None, help="a checkpoint directory (config.json + model.safetensors) instead of a fixture")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--tokens", type=int, default=2048)
    ap.add_argument("--ctx-tokens", type=int, default=257)
    ap.add_argument("--seed", type=int, default=4321)
    ap.add_argument("--steps", type=int, default=0, help="sampler steps of the loop comparison (0: the forward only)")
    ap.add_argument("--modes", default="bf16,float16,fp8,fp8_fast")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    modes = [m for m in a.modes.split(",") if m]
    for m in modes:
        if m not in MODES:
            ap.error(f"--modes: {m!r} is none of {sorted(MODES)}")
    if not a.case and not a.weights:
        ap.error("give --case NAME (repeatable) or --weights DIR")
    if not torch.cuda.is_available():
        raise SystemExit("stage1_fp32_probe: needs a GPU (there is no CPU path)")
    dev = torch.device(a.device)
    doc = dict(tool="tools/stage1_fp32_probe.py", device=torch.cuda.get_device_name(dev), guidance=GUIDANCE, scales=SCALES, forward_t=FWD_T,
               cases=[])

    def record(rec):                                    # written after every case: a long run keeps what it has
        doc["cases"].append(rec)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")
    with torch.no_grad():
        for spec in a.case:
            name, _, steps = spec.partition(":")
            record(probe(name, fixture_case(name), modes, int(steps) if steps else a.steps, dev))
        if a.weights:
            case = checkpoint_case(a.weights, a.frames, a.tokens, a.ctx_tokens, a.seed)
            record(probe(os.path.basename(os.path.normpath(a.weights)), case, modes, a.steps, dev))
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
