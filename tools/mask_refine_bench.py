"""Time the mask refinement: the device path against the scipy restatement of the reference's `refine_mask`.

    python tools/mask_refine_bench.py [--frames 16] [--size 512] [--reps 60] [--warmup 5] [--out profiles/mask_refine.json]

One process, one GPU.  The clip: `frames` frames of size x size, each a soft blob plus noise, uint8, seeded (tests/test_components_gpu.py's
`soft_blob`).  Per repetition, alternating:
  * `refine_masks` on the device-resident clip (zero, histogram, Otsu, tile labelling, border merge, flatten, output: seven launches
    for the whole clip) between two HIP events on the current stream, and by a host clock around the same call plus a synchronise;
  * the host restatement of `refine_mask` frame after frame - `otsu_threshold`, `scipy.ndimage.label` with the full structure,
    `np.bincount`, the size rule - by a host clock on the same box.  This is the RESTATEMENT's time, not cv2's / skimage's: neither
    is installable where this was written.
Before timing, the device masks are compared with the restatement's, bit for bit.  Recorded, not gated.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def summary(xs):
    xs = sorted(xs)
    return {"n": len(xs), "median_ms": statistics.median(xs), "min_ms": xs[0], "max_ms": xs[-1],
            "p10_ms": xs[len(xs) // 10], "p90_ms": xs[(len(xs) * 9) // 10]}


def host_refine(frame, min_size):
    """What the reference's refine_mask computes, restated: threshold, 8-connected labels, sizes, the size rule."""
    from scipy import ndimage
    from actionmesh_amd.mask_refine import otsu_threshold
    lab, n = ndimage.label(frame > int(otsu_threshold(frame)), structure=np.ones((3, 3), int))
    big = np.bincount(lab.reshape(-1), minlength=n + 1) >= min_size
    big[0] = False
    return np.where(big[lab], 255, 0).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--min-size", type=int, default=200)
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_refine.json"))
    args = ap.parse_args()
    from actionmesh_amd import mask_refine as MR
    from test_components_gpu import soft_blob

    clip_host = np.stack([soft_blob(args.size, args.size, seed) for seed in range(args.frames)])
    clip = torch.from_numpy(clip_host).cuda()
    got, stats = MR.refine_masks(clip, min_size=args.min_size, return_stats=True)
    want = np.stack([host_refine(f, args.min_size) for f in clip_host])
    identical = bool(np.array_equal(got.cpu().numpy(), want))
    hip_ms, hip_wall_ms, host_ms = [], [], []
    for rep in range(args.warmup + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        MR.refine_masks(clip, min_size=args.min_size)
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for f in clip_host:
            host_refine(f, args.min_size)
        t2 = time.perf_counter()
        if rep >= args.warmup:
            hip_ms.append(e0.elapsed_time(e1))
            hip_wall_ms.append((t1 - t0) * 1e3)
            host_ms.append((t2 - t1) * 1e3)
    rec = {"what": "mask refinement (Otsu, 8-connected components, small-object removal): device path vs the scipy restatement of "
                   "the reference's refine_mask, alternating in one process",
           "clip": f"{args.frames} frames of {args.size} x {args.size}, soft blob + noise, seeds 0..{args.frames - 1}",
           "min_size": args.min_size, "stats_threshold_foreground_components_kept": stats.cpu().tolist(),
           "bit_identical_to_restatement": identical, "warmup": args.warmup,
           "hip_refine_masks_event": summary(hip_ms), "hip_refine_masks_host_clock": summary(hip_wall_ms),
           "scipy_restatement_host_clock": summary(host_ms),
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cpu_threads": torch.get_num_threads(),
           "note": "the host figure is the restatement's (numpy Otsu loop + scipy.ndimage.label + np.bincount, frame after frame, "
                   "single-threaded by nature), not cv2's / skimage's; the hip figures cover the whole clip in one call and include the "
                   "workspace allocation from torch's caching allocator"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
