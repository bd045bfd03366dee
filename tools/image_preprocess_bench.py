"""Time the frame preprocessing in front of DINOv2: the device path against the "pil" half it replaces.

    python tools/image_preprocess_bench.py [--clip davis_camel] [--reps 50] [--warmup 5] [--out profiles/image_preprocess.json]

One process, one GPU.  Per repetition, alternating:
  * `frames_to_pixel_values` (raw RGBA frames on the device -> pixel_values: alpha statistics, the one host read, crop geometry,
    horizontal and vertical pass) between two HIP events on the current stream;
  * the preprocessing half of `HipImageEncoder.encode_images` on the "pil" path - `BitImageProcessor.preprocess` on the PIL frames
    `process_images` returns, and the upload of pixel_values - by a host clock (it is CPU work) on the same box.
The reference's `ImagePreprocessor.process_images` has no counterpart outside the reference checkout and is not timed here.
Recorded, not gated: the JSON holds every sample's summary and the call's environment.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

DINO_CONFIG = {"crop_size": {"height": 224, "width": 224}, "do_center_crop": True, "do_convert_rgb": True, "do_normalize": True,
               "do_rescale": True, "do_resize": True, "image_mean": [0.485, 0.456, 0.406], "image_std": [0.229, 0.224, 0.225],
               "resample": 3, "rescale_factor": 0.00392156862745098, "size": {"shortest_edge": 256}}


def summary(xs):
    xs = sorted(xs)
    return {"n": len(xs), "median_ms": statistics.median(xs), "min_ms": xs[0], "max_ms": xs[-1],
            "p10_ms": xs[len(xs) // 10], "p90_ms": xs[(len(xs) * 9) // 10]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clip", default="davis_camel")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_preprocess.json"))
    args = ap.parse_args()
    from PIL import Image
    from transformers import BitImageProcessor
    from actionmesh_amd import image_preprocess as IP
    from make_golden_frames_raw import load_clip

    raw_host = load_clip(args.clip)
    raw = torch.from_numpy(raw_host).cuda()
    settings = IP.processor_settings(DINO_CONFIG)
    pil_frames = IP.HipImagePreprocessor().process_images([Image.fromarray(f) for f in raw_host])
    proc = BitImageProcessor(**DINO_CONFIG)
    want = proc.preprocess(pil_frames, return_tensors="pt").pixel_values
    got = IP.frames_to_pixel_values(raw, settings)
    identical = bool(torch.equal(got.cpu(), want))
    hip_ms, hip_wall_ms, pil_ms = [], [], []
    for rep in range(args.warmup + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        IP.frames_to_pixel_values(raw, settings)
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        pix = proc.preprocess(pil_frames, return_tensors="pt").pixel_values.cuda()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        del pix
        if rep >= args.warmup:
            hip_ms.append(e0.elapsed_time(e1))
            hip_wall_ms.append((t1 - t0) * 1e3)
            pil_ms.append((t2 - t1) * 1e3)
    rec = {"what": "frame preprocessing in front of DINOv2: device path vs the encoder's 'pil' half, alternating in one process",
           "clip": args.clip, "frames": list(raw_host.shape), "processor": "shortest_edge 256 bicubic, centre crop 224",
           "bit_identical_to_pil_path": identical, "warmup": args.warmup,
           "hip_frames_to_pixel_values_event": summary(hip_ms), "hip_frames_to_pixel_values_host_clock": summary(hip_wall_ms),
           "pil_bitimageprocessor_plus_upload_host_clock": summary(pil_ms),
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "cpu_threads": torch.get_num_threads(),
           "note": "the hip figure includes the device-to-host read of the alpha statistics and the host-side geometry; "
                   "ImagePreprocessor.process_images (reference only) is not timed here"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
