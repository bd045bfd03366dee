"""Per-launch time of the exact-fp32 kernels at Stage II's shipped shapes (run it under `rocprofv3 --kernel-trace --stats` for the
kernel-only times DESIGN.md records; the event times printed here include launch overhead):
  am_gemm_f32 at M = 50 000, (N, K) in {(1024, 1024), (4096, 1024), (1024, 4096)};
  am_attention_f32 at (nseq, H, sq, sk) = (1, 8, 50 000, 32 784), head_dim 128, the cross-attention's [to_k | to_v] layout."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from actionmesh_amd import ops  # noqa: E402


def _time(fn, reps):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--vertices", type=int, default=50000)
    ap.add_argument("--keys", type=int, default=32784)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    M = a.vertices
    for N, K in ((1024, 1024), (4096, 1024), (1024, 4096)):
        x = torch.randn((M, K), generator=g, device=dev)
        w = torch.randn((N, K), generator=g, device=dev)
        out = torch.empty((M, N), device=dev)
        ms = _time(lambda: ops.gemm_f32(x, w, out=out), a.reps)
        print(json.dumps({"kernel": "am_gemm_f32", "M": M, "N": N, "K": K, "ms": round(ms, 3), "tflops": round(2.0 * M * N * K / ms / 1e9, 1)}))
        del x, w, out
    H, D, S = 8, 128, a.keys
    q = torch.randn((M, H * D), generator=g, device=dev)
    kv = torch.randn((S, 2 * H * D), generator=g, device=dev)
    out = torch.empty((M, H * D), device=dev)
    ms = _time(lambda: ops.attention_f32(q, kv, kv, H, M, S, D, k_hs=2 * D, v_hs=2 * D, v_off=D, out=out), max(1, a.reps // 2))
    print(json.dumps({"kernel": "am_attention_f32", "nseq": 1, "heads": H, "sq": M, "sk": S, "head_dim": D, "ms": round(ms, 3),
                      "tflops": round(4.0 * M * S * H * D / ms / 1e9, 1)}))


if __name__ == "__main__":
    main()
