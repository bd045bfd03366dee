#!/usr/bin/env python
"""Times the fused ICP iteration (csrc/am_icp.hip, gradient_icp(step="fused")) against the autograd path on one MI355X.  Everything runs
in ONE process, the methods alternate call by call, and every figure is a median with its minimum and maximum (wall clock around a
device synchronisation), as in tools/nn_grid_timing.py, whose `alternating` and `summary` this file reuses:

  * a whole gradient_icp of --icp_iter iterations (default the reference's 200) at 10 000 x 10 000 points, surface samples of an
    ellipsoid, on aligned inputs (the target a slightly moved copy) and on canonically-rotated ones (the similarity the ICP test
    recovers): autograd over brute-force searches, autograd over grid searches, and fused;
  * beside them, on the same clouds, the 2 x icp_iter brute-force fp32 searches of one ICP with nothing between them: what the
    autograd path spends outside its searches, measured and not inferred;
  * evaluate_sample on a synthetic 16-frame sequence (10 000 ICP points, 100 000 metric points), autograd against fused.

The last block states which method the whole-ICP timing favours and by how much against the spread between repeats.  Writes
profiles/icp_fused.json; no test asserts a time, and no default follows from it (actionbench.EVALUATOR_ICP stays "autograd").

    python tools/icp_timing.py [--out profiles/icp_fused.json] [--icp_iter 200] [--icp_repeats 5] [--skip_eval]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from nn_grid_timing import alternating, ellipsoid  # noqa: E402


def icp_case(name, pred, gt, n_iter, repeats, dev):
    from actionmesh_amd import actionbench as AB
    from actionmesh_amd import ops
    res = {}
    R_init = AB.canonical_rotation_matrices().to(dev)
    moved = (pred[None] @ R_init).contiguous()                 # 24 clouds of the size the ICP searches against

    def run(key, **kw):
        res[key] = AB.gradient_icp(pc_pred=pred, pc_gt=gt, n_iter=n_iter, **kw)

    def searches():
        for _ in range(n_iter):
            ops.nearest_neighbors(gt, moved, precise=False, check=False)
            ops.nearest_neighbors(moved, gt, precise=False, check=False)

    t = alternating({"autograd_brute": lambda: run("autograd_brute", nn="brute"), "autograd_grid": lambda: run("autograd_grid", nn="grid"),
                     "fused": lambda: run("fused", step="fused"), "searches_only": searches}, repeats, 1, dev)
    assert res["autograd_brute"].loss == res["autograd_grid"].loss
    icp = {k: t[k] for k in ("autograd_brute", "autograd_grid", "fused")}
    spread = max(v["max_ms"] - v["min_ms"] for v in icp.values())
    best_auto = min(("autograd_brute", "autograd_grid"), key=lambda k: t[k]["median_ms"])
    diff = t[best_auto]["median_ms"] - t["fused"]["median_ms"]
    row = {"case": name, "points": [int(pred.shape[0]), int(gt.shape[0])], "n_iter": n_iter, **t,
           "loss": {k: v.loss for k, v in res.items()},
           "autograd_brute_minus_searches_ms": round(t["autograd_brute"]["median_ms"] - t["searches_only"]["median_ms"], 3),
           "fused_minus_searches_ms": round(t["fused"]["median_ms"] - t["searches_only"]["median_ms"], 3),
           "spread_ms": round(spread, 3), "faster_autograd": best_auto, "faster_autograd_minus_fused_ms": round(diff, 3),
           "favours": "fused" if diff > spread else best_auto if -diff > spread else "neither (inside the spread)"}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_fused.json"))
    ap.add_argument("--icp_iter", type=int, default=200)
    ap.add_argument("--icp_repeats", type=int, default=5)
    ap.add_argument("--eval_repeats", type=int, default=2)
    ap.add_argument("--skip_eval", action="store_true")
    a = ap.parse_args()
    from actionmesh_amd import actionbench as AB
    from actionmesh_amd import mesh_io
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "gradient_icp": []}

    pred = ellipsoid(10_000, 5, dev)
    aligned = (pred[torch.randperm(10_000, generator=torch.Generator().manual_seed(2)).to(dev)] * 1.01 + 0.002).contiguous()
    out["gradient_icp"].append(icp_case("aligned", pred, aligned, a.icp_iter, a.icp_repeats, dev))
    R_true = AB.canonical_rotation_matrices()[9].to(dev) @ AB.euler_angles_to_matrix(torch.tensor([0.21, -0.1, 0.05])).to(dev)
    gt = ((torch.tensor([1.1, 0.95, 1.05], device=dev) * ellipsoid(10_000, 6, dev)) @ R_true + torch.tensor([0.05, -0.02, 0.03], device=dev)).contiguous()
    out["gradient_icp"].append(icp_case("canonically_rotated", pred, gt, a.icp_iter, a.icp_repeats, dev))

    if not a.skip_eval:
        from _decimate_ref import icosphere
        v0, f = icosphere(4)
        with tempfile.TemporaryDirectory() as tmp:
            frames = [v0 * [1.0, 0.7, 0.5] * (1.0 + 0.02 * k) + [0.01 * k, 0.0, 0.0] for k in range(16)]
            os.makedirs(os.path.join(tmp, "pred", "seq"))
            os.makedirs(os.path.join(tmp, "gt", "seq"))
            for k, v in enumerate(frames):
                mesh_io.save_glb(v.astype(np.float32), f, os.path.join(tmp, "pred", "seq", f"mesh_{k:02d}.glb"))
            gt_v = torch.from_numpy(np.stack(frames)).float().to(dev) * torch.tensor([1.05, 0.97, 1.02], device=dev) + 0.02
            surf = AB.sample_meshes(gt_v, torch.from_numpy(f).to(dev), n_pts=100_000, synchronized=True, seed=9)
            np.save(os.path.join(tmp, "gt", "seq", "surfaces.npy"), surf.cpu().numpy())
            got = {}

            def ev(icp):
                r = AB.evaluate_sample("seq", os.path.join(tmp, "gt"), os.path.join(tmp, "pred"), device="cuda", n_iter=a.icp_iter, icp=icp)
                assert r.status == "success", r.error_message
                got[icp] = {"cd_3d": r.cd_3d, "cd_4d": r.cd_4d, "cd_motion": r.cd_motion}

            t = alternating({"autograd": lambda: ev("autograd"), "fused": lambda: ev("fused")}, a.eval_repeats, 0, dev)
            out["evaluate_sample_16_frames"] = {k: {**t[k], **got[k]} for k in t}
            print(json.dumps(out["evaluate_sample_16_frames"]), flush=True)

    # which method the whole-ICP timing favours, and by how much against the spread between repeats
    out["verdict"] = [{"case": r["case"], "favours": r["favours"], "faster_autograd": r["faster_autograd"],
                       "faster_autograd_minus_fused_ms": r["faster_autograd_minus_fused_ms"], "spread_ms": r["spread_ms"]}
                      for r in out["gradient_icp"]]
    print(json.dumps(out["verdict"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
