"""How far are the 16-bit Stage-II modes from fp32 - measured against the DEVICE fp32 run, HipAutoencoder(exact_fp32=True).

One process, one device.  Per case the exact model and the 16-bit models are built from the same weights and inputs:
  * a fixture name (`--case ae_tiny`, `--case ae_arch`): the seeded weights of oracle.autoencoder_oracle and the inputs stored in
    tests/golden/<name>.npz, with the reference's own fp32 displacement beside them;
  * `--case shipped`: the shipped architecture (width 1024, 8 heads, 16 + 1 blocks) with seeded weights and seeded inputs of
    `--frames` x `--tokens` latent tokens, `--targets` target timesteps and `--vertices` query vertices;
  * or a checkpoint directory (`--weights DIR`, read with from_pretrained: config.json + model.safetensors) with seeded inputs of the
    same four flags - a user's own check of their own weights.
The exact mode runs ONCE per case; then every other mode runs against it: bf16 and float16, each with residual_fp32=False, the default,
and cross_fp32=True.  Reported per case, as one JSON document (`--out`, and stdout):
  (a) per mode the displacement's rel-L2 and the maximum per-vertex Euclidean error against the device fp32 run (and, where the fixture
      exists, against the reference's fp32 displacement);
  (b) where the fixture exists: the device fp32 run against the reference's fp32 displacement, rel-L2 and max-abs;
  (c) the wall time per window (one forward over all targets) around a device synchronisation, weights uploaded beforehand: the exact
      mode's one run, and the second of two runs of each 16-bit mode; the exact mode's algorithmic work beside it.

    python tools/stage2_fp32_probe.py --case ae_tiny --case ae_arch --case shipped --out profiles/stage2_fp32.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from actionmesh_amd import HipAutoencoder  # noqa: E402
from oracle import autoencoder_oracle as AO  # noqa: E402

MODES = {f"{name}{suffix}": dict(dtype=dt, **kw) for name, dt in (("bf16", "bfloat16"), ("float16", "float16"))
         for suffix, kw in (("_residual16", dict(residual_fp32=False)), ("", {}), ("_cross_fp32", dict(cross_fp32=True)))}
FIELDS = ("temporal_context_size", "in_channels", "in_extra_channels", "out_dim", "latent_channels", "width", "num_layers", "embed_frequency",
          "embed_include_pi", "prediction_mode")


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def vertex_error(a, b):
    """The largest Euclidean distance between a vertex's two displacements."""
    return float((a.double() - b.double()).norm(dim=-1).max())


def seeded_inputs(T, N, T_out, V, D, extra, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.rand((1, V, 3), generator=g) * 2 - 1
    if extra:
        q = torch.cat([q, torch.nn.functional.normalize(torch.randn((1, V, extra), generator=g), dim=-1)], -1)
    return dict(latent=torch.randn((1, T, N, D), generator=g), framestep=torch.arange(T, dtype=torch.float32)[None],
                source_alpha=torch.zeros(1), target_alphas=torch.linspace(0.0, 1.0, T_out + 1)[None, 1:].contiguous(), query=q)


def fixture_case(name):
    """(make(**kw) -> HipAutoencoder on the CPU, inputs, the reference's fp32 displacement)"""
    g = np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))
    width, layers, heads, latent = (int(v) for v in g["config"])
    cfg = AO.AEConfig(width=width, num_layers=layers, num_attention_heads=heads, latent_channels=latent)
    sd = AO.synthetic_state_dict(cfg, seed=0)
    inp = {k: torch.from_numpy(g[k]) for k in ("latent", "framestep", "source_alpha", "target_alphas", "query")}
    return _maker(dict(width=width, num_layers=layers, num_attention_heads=heads, latent_channels=latent), sd), inp, torch.from_numpy(g["displacement_fp32"])


def shipped_case(a):
    cfg = AO.AEConfig()
    sd = AO.synthetic_state_dict(cfg, seed=0)
    fields = dict(width=cfg.width, num_layers=cfg.num_layers, num_attention_heads=cfg.num_attention_heads, latent_channels=cfg.latent_channels)
    return _maker(fields, sd), seeded_inputs(a.frames, a.tokens, a.targets, a.vertices, cfg.latent_channels, cfg.in_extra_channels, a.seed), None


def checkpoint_case(path, a):
    probe = HipAutoencoder.from_pretrained(path)
    fields = {k: getattr(probe, k) for k in FIELDS}
    fields["num_attention_heads"] = probe.heads
    return (_maker(fields, probe._sd),
            seeded_inputs(a.frames, a.tokens, a.targets, a.vertices, probe.latent_channels, probe.in_extra_channels, a.seed), None)


def _maker(fields, sd):
    def make(**model_kw):
        m = HipAutoencoder(**fields, **model_kw)
        m.load_state_dict(sd)
        return m
    return make


def window(model, inp, dev):
    """One forward over all targets; (displacement on the CPU, seconds around a synchronise)."""
    args = (inp["latent"].to(dev), inp["framestep"], inp["source_alpha"], inp["target_alphas"], inp["query"].to(dev))
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    d = model(*args)
    torch.cuda.synchronize(dev)
    return d.float().cpu(), time.perf_counter() - t0


def window_flops(model, B, T, N, T_out, V):
    """Multiply-adds x 2 of one exact window: the linears and the two matrix products of every attention."""
    C, NL, S = model.width, model.num_layers, T * (N + 1)
    rows = B * S
    self_block = 24 * rows * C * C + 4 * B * S * S * C
    cross = 4 * rows * C * C + B * V * (20 * C * C + 4 * S * C)
    return float(T_out * (NL * self_block + cross))


def probe(label, case, dev):
    make, inp, ref = case
    B, T, N, _ = inp["latent"].shape
    T_out, V = inp["target_alphas"].shape[1], inp["query"].shape[1]
    m32 = make(exact_fp32=True).to(dev).eval()
    rec = dict(case=label, frames=T, tokens=N, targets=T_out, vertices=V, width=m32.width, layers=m32.num_layers,
               window_flops=window_flops(m32, B, T, N, T_out, V))
    m32._w32_self, m32._w32                                                               # the fp32 weights, uploaded before the clock starts
    d32, sec = window(m32, inp, dev)
    rec["fp32_window_seconds"] = sec
    rec["fp32_window_tflops"] = rec["window_flops"] / sec / 1e12
    rec["fp32_entry_counts"] = m32.entry_counts()
    print(f"[{label}] exact fp32 window {sec:.3f} s, {rec['fp32_window_tflops']:.1f} TFLOP/s algorithmic", flush=True)
    if ref is not None:                                                                   # (b)
        rec["fp32_vs_reference_fp32"] = dict(rel_l2=rel(d32, ref), max_abs=float((d32 - ref).abs().max()), max_vertex_error=vertex_error(d32, ref))
        print(f"[{label}] device fp32 vs the reference's fp32 displacement: {rec['fp32_vs_reference_fp32']}", flush=True)
    m32.to("cpu")
    del m32
    torch.cuda.empty_cache()
    rec["modes"] = {}
    for mode, kw in MODES.items():                                                        # (a), (c)
        m = make(**kw).to(dev).eval()
        window(m, inp, dev)
        d, sec = window(m, inp, dev)
        r = dict(rel_l2_vs_device_fp32=rel(d, d32), max_vertex_error_vs_device_fp32=vertex_error(d, d32), window_seconds=sec)
        if ref is not None:
            r["rel_l2_vs_reference_fp32"] = rel(d, ref)
            r["max_vertex_error_vs_reference_fp32"] = vertex_error(d, ref)
        m.to("cpu")
        del m
        torch.cuda.empty_cache()
        rec["modes"][mode] = r
        print(f"[{label}] {mode}: rel-L2 vs device fp32 {r['rel_l2_vs_device_fp32']:.4e}, max per-vertex error "
              f"{r['max_vertex_error_vs_device_fp32']:.4e}, window {sec:.3f} s", flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--case", action="append", default=[], metavar="NAME",
                    help="ae_tiny / ae_arch (fixtures of tests/golden) or shipped (seeded weights at the shape flags); repeatable")
    ap.add_argument("--weights", default=None, help="a checkpoint directory (config.json + model.safetensors) instead of a fixture")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--tokens", type=int, default=2048)
    ap.add_argument("--targets", type=int, default=15)
    ap.add_argument("--vertices", type=int, default=50000)
    ap.add_argument("--seed", type=int, default=4321)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not a.case and not a.weights:
        ap.error("give --case NAME (repeatable) or --weights DIR")
    if not torch.cuda.is_available():
        raise SystemExit("stage2_fp32_probe: needs a GPU (there is no CPU path)")
    dev = torch.device(a.device)
    doc = dict(tool="tools/stage2_fp32_probe.py", device=torch.cuda.get_device_name(dev), seed=a.seed, cases=[])

    def record(rec):                                    # written after every case: a long run keeps what it has
        doc["cases"].append(rec)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")
    for name in a.case:
        record(probe(name, shipped_case(a) if name == "shipped" else fixture_case(name), dev))
    if a.weights:
        record(probe(os.path.basename(os.path.normpath(a.weights)), checkpoint_case(a.weights, a), dev))
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
