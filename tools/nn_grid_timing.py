#!/usr/bin/env python
"""Times the grid nearest-neighbour search (csrc/am_nn_grid.hip) against the brute-force kernel (am_nn_search, which this search does
not touch) on one MI355X.  The methods alternate call by call in ONE process, every figure is a median with its minimum and maximum
(wall clock around a device synchronisation), and the grid's build and search are timed separately as well as together:

  * 24 x 10 000 x 10 000 in fp32 - the ICP's inner search - on surface samples of an ellipsoid: the queries a slightly moved copy
    (aligned), and the queries turned into the 24 canonical orientations (what the ICP's candidates look like at its start);
  * 100 000 x 10 000 and 100 000 x 100 000 in fp64 - the metric's searches - aligned;
  * each with G at 1/2, 1 and 2 times the default clamp(ceil(cbrt(2 P)), 1, 128);
  * a whole gradient_icp of --icp_iter iterations (default the reference's 200), brute force against the grid;
  * evaluate_sample on a synthetic 16-frame sequence (10 000 ICP points, 100 000 metric points), brute force against the grid.

The last block of the output states which method the whole-gradient_icp timing favours and by how much against the spread between
repeats: the evaluator's default (actionbench.EVALUATOR_NN) follows it.  Writes profiles/nn_grid.json; no test asserts a time.

    python tools/nn_grid_timing.py [--out profiles/nn_grid.json] [--repeats 7] [--icp_iter 200] [--skip_eval]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def summary(times):
    return {"median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4), "n": len(times)}


def alternating(fns, repeats, warmup, dev):
    """one call of each callable per round, so that drift of the clocks or of the box hits all alike"""
    times = {name: [] for name in fns}
    for k in range(warmup + repeats):
        for name, fn in fns.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            if k >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    return {name: summary(t) for name, t in times.items()}


def ellipsoid(n, seed, dev, batch=None):
    g = torch.Generator().manual_seed(seed)
    u = torch.randn((n, 3) if batch is None else (batch, n, 3), generator=g)
    return (u / u.norm(dim=-1, keepdim=True) * torch.tensor([1.0, 0.7, 0.4])).to(dev)


def search_case(name, points, queries, precise, repeats, dev, cells_factors=(0.5, 1.0, 2.0)):
    from actionmesh_amd import ops
    P = points.shape[-2]
    G0 = ops.nn_grid_default_cells(P)
    ref = ops.nearest_neighbors(points, queries, precise=precise)
    row = {"case": name, "points": list(points.shape), "queries": list(queries.shape), "precision": "fp64" if precise else "fp32",
           "default_cells": G0, "grid": []}
    fns = {"brute": lambda: ops.nearest_neighbors(points, queries, precise=precise, check=False)}
    own = ops.nn_grid_build(queries).order                      # the query cloud's own cell order (the ICP has it for free)
    for fct in cells_factors:
        G = min(max(int(round(G0 * fct)), 1), 128)
        grid = ops.nn_grid_build(points, cells=G)
        got = ops.nn_grid_search(grid, queries, precise=precise, query_order=own)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1].view(torch.uint8), ref[1].view(torch.uint8)), (name, G)
        fns[f"build_G{G}"] = lambda G=G: ops.nn_grid_build(points, cells=G)
        fns[f"search_G{G}"] = lambda grid=grid: ops.nn_grid_search(grid, queries, precise=precise, query_order=own, check=False)
        fns[f"search_unordered_G{G}"] = lambda grid=grid: ops.nn_grid_search(grid, queries, precise=precise, check=False)
        fns[f"build_and_search_G{G}"] = lambda G=G: ops.nn_grid_search(ops.nn_grid_build(points, cells=G), queries, precise=precise,
                                                                        query_order=own, check=False)
    t = alternating(fns, repeats, 2, dev)
    row["brute"] = t.pop("brute")
    row["grid"] = t
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nn_grid.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--icp_iter", type=int, default=200)
    ap.add_argument("--icp_repeats", type=int, default=3)
    ap.add_argument("--skip_eval", action="store_true")
    a = ap.parse_args()
    from actionmesh_amd import actionbench as AB
    from actionmesh_amd import mesh_io
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "searches": []}

    cloud = ellipsoid(10_000, 1, dev)
    aligned = (cloud[torch.randperm(10_000, generator=torch.Generator().manual_seed(2)).to(dev)] * 1.01 + 0.002)
    out["searches"].append(search_case("icp_aligned_24x10k_x_10k", cloud, aligned[None].repeat(24, 1, 1).contiguous(), False, a.repeats, dev))
    R = AB.canonical_rotation_matrices().to(dev)
    out["searches"].append(search_case("icp_24_orientations_24x10k_x_10k", cloud, (aligned[None] @ R).contiguous(), False, a.repeats, dev))
    # the other direction of the ICP: 24 grids, rebuilt per iteration, queried by the shared cloud
    out["searches"].append(search_case("icp_24_orientations_24_grids", (aligned[None] @ R).contiguous(), cloud, False, a.repeats, dev))
    big = ellipsoid(100_000, 3, dev)
    near = big[torch.randperm(100_000, generator=torch.Generator().manual_seed(4)).to(dev)] * 1.01 + 0.002
    out["searches"].append(search_case("metric_100k_x_10k", big, near[:10_000].contiguous(), True, a.repeats, dev))
    out["searches"].append(search_case("metric_100k_x_100k", big, near.contiguous(), True, a.repeats, dev))

    # a whole gradient_icp: the similarity the ICP test recovers, at the reference's 10 000 points
    pred = ellipsoid(10_000, 5, dev)
    R_true = AB.canonical_rotation_matrices()[9].to(dev) @ AB.euler_angles_to_matrix(torch.tensor([0.21, -0.1, 0.05])).to(dev)
    gt = (torch.tensor([1.1, 0.95, 1.05], device=dev) * ellipsoid(10_000, 6, dev)) @ R_true + torch.tensor([0.05, -0.02, 0.03], device=dev)
    res = {}

    def icp(nn):
        res[nn] = AB.gradient_icp(pc_pred=pred, pc_gt=gt, n_iter=a.icp_iter, nn=nn)

    t = alternating({"brute": lambda: icp("brute"), "grid": lambda: icp("grid")}, a.icp_repeats, 1, dev)
    assert res["brute"].loss == res["grid"].loss and torch.equal(res["brute"].R, res["grid"].R)
    spread = max(v["max_ms"] - v["min_ms"] for v in t.values())
    diff = t["brute"]["median_ms"] - t["grid"]["median_ms"]
    choice = "grid" if diff > spread else "brute"
    out["gradient_icp"] = {"points": 10_000, "n_iter": a.icp_iter, "loss": res["grid"].loss, **t, "spread_ms": round(spread, 3),
                           "brute_minus_grid_ms": round(diff, 3), "evaluator_default": choice}
    print(json.dumps(out["gradient_icp"]), flush=True)

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
            ev = {}
            for nn in ("brute", "grid"):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                r = AB.evaluate_sample("seq", os.path.join(tmp, "gt"), os.path.join(tmp, "pred"), device="cuda", n_iter=a.icp_iter, nn=nn)
                torch.cuda.synchronize(dev)
                assert r.status == "success", r.error_message
                ev[nn] = {"seconds": round(time.perf_counter() - t0, 3), "cd_3d": r.cd_3d, "cd_4d": r.cd_4d, "cd_motion": r.cd_motion}
            assert all(ev["brute"][k] == ev["grid"][k] for k in ("cd_3d", "cd_4d", "cd_motion"))
            out["evaluate_sample_16_frames"] = ev
            print(json.dumps(ev), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
