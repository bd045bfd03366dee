#!/usr/bin/env python
"""Times the mesh decimation (actionmesh_amd/mesh_decimate.py over csrc/am_decimate.hip) on one MI355X: a noisy sphere - an
octahedron subdivided n times along every edge, 8 n^2 faces, projected to the unit sphere, every vertex moved by 0.2 mean edge
lengths of seeded noise - decimated to 40 000 faces from about 400 000 (n = 224) and about 100 000 (n = 112).  Per case: the number
of rounds, the time of one `decimate_mesh` call (wall clock around a device synchronisation, median of 20 after 3 warm-up calls)
and that time over the rounds.

`fast_simplification`, which the reference decimates with, is not installable offline, so there is no figure of it here.  The only host
figure is the tests' own SEQUENTIAL GREEDY RESTATEMENT in numpy (tests/_decimate_ref.py greedy_decimate: a heap, one collapse at a
time, the tables rebuilt after every collapse) on the tests' small meshes - a yardstick for the tests' quality bound, not an
implementation anyone would ship, and labelled as that in the output.

`--quality` needs no GPU: it re-measures the surface-distance ratios that tests/test_mesh_decimate_cpu.py bounds (round scheme
over sequential greedy, both through the numpy restatement) and stores them, with the seconds the greedy restatement took, under
"quality".

`--borders collapse` measures `decimate_mesh(..., borders="collapse")` instead and writes the "timing" section of
profiles/mesh_decimate_borders.json: on the closed noisy sphere the two modes ALTERNATE in one process (the outputs are the same
bits, so the difference is the price of am_decimate_border_edges and of the prefix trimming on a mesh without border), then the same
sphere with one cap cut off (the faces whose centroid has z > 0.8): rounds and time with "collapse", and where "fixed" stops.

Writes profiles/mesh_decimate.json, keeping the sections it does not measure; no test asserts a time.

    python tools/mesh_decimate_timing.py [--out profiles/mesh_decimate.json] [--quality] [--borders collapse]
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


def noisy_sphere(n: int, noise: float = 0.2, seed: int = 0):
    """(vertices (4 n^2 + 2, 3) fp64, faces (8 n^2, 3) int64): the octahedron |x| + |y| + |z| = n on the integer lattice, one octant at a
    time, merged on the integer coordinates, outward winding."""
    a, b = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    keep = a + b <= n
    a, b = a[keep], b[keep]
    index = -np.ones((n + 1, n + 1), dtype=np.int64)
    index[a, b] = np.arange(a.size)
    up = (a + b < n)
    down = (a + b < n - 1)
    tri = np.concatenate((np.stack((index[a[up], b[up]], index[a[up] + 1, b[up]], index[a[up], b[up] + 1]), 1),
                          np.stack((index[a[down] + 1, b[down]], index[a[down] + 1, b[down] + 1], index[a[down], b[down] + 1]), 1)))
    lattice = np.stack((a, b, n - a - b), 1)
    points, faces = [], []
    for k, sign in enumerate(np.array(np.meshgrid((1, -1), (1, -1), (1, -1), indexing="ij")).reshape(3, -1).T):
        points.append(lattice * sign)
        faces.append((tri if sign.prod() > 0 else tri[:, ::-1]) + k * a.size)
    uniq, inverse = np.unique(np.concatenate(points), axis=0, return_inverse=True)
    f = inverse.reshape(-1)[np.concatenate(faces)]
    v = uniq / np.linalg.norm(uniq, axis=1, keepdims=True)
    edge = np.linalg.norm(v[f[:, 0]] - v[f[:, 1]], axis=1).mean()
    return v + np.random.default_rng(seed).normal(scale=noise * edge / 3 ** 0.5, size=v.shape), f


def timed(fn, repeats, warmup, dev):
    times = []
    for k in range(warmup + repeats):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        if k >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(times), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3), "n": repeats}


def cut_cap(v, f, z=0.8):
    """The mesh without the faces whose centroid lies above z, unused vertices dropped: an open mesh with one border loop."""
    f = f[v[f].mean(1)[:, 2] <= z]
    used = np.unique(f)
    remap = np.full(v.shape[0], -1, dtype=np.int64)
    remap[used] = np.arange(used.shape[0])
    return v[used], remap[f]


def border_timing(n, target, dev, repeats=20, warmup=3):
    from actionmesh_amd import mesh_decimate as MD
    v, f = noisy_sphere(n)
    rows = {}
    for name, (mv, mf) in (("closed", (v, f)), ("cap_cut_off", cut_cap(v, f))):
        verts, faces = torch.from_numpy(mv).float().to(dev), torch.from_numpy(mf).to(dev)
        results = {b: MD.decimate_mesh(verts, faces, target, return_rounds=True, borders=b) for b in ("fixed", "collapse")}
        times = {"fixed": [], "collapse": []}
        for k in range(warmup + repeats):                  # the two modes alternate: what drifts, drifts for both
            for b in ("fixed", "collapse"):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                MD.decimate_mesh(verts, faces, target, borders=b)
                torch.cuda.synchronize(dev)
                if k >= warmup:
                    times[b].append((time.perf_counter() - t0) * 1e3)
        row = {"subdivisions": n, "vertices": int(mv.shape[0]), "faces": int(mf.shape[0]), "target_faces": target,
               "same_bits": all(torch.equal(x, y) for x, y in zip(results["fixed"][:2], results["collapse"][:2]))
               if results["fixed"][1].shape == results["collapse"][1].shape else False}
        for b in ("fixed", "collapse"):
            t = times[b]
            row[b] = {"faces_after": int(results[b][1].shape[0]), "rounds": results[b][2], "median_ms": round(statistics.median(t), 3),
                      "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "n": repeats,
                      "ms_per_round": round(statistics.median(t) / max(results[b][2], 1), 3)}
        rows[name] = row
        print(json.dumps({name: row}))
    return {"what": "decimate_mesh on the noisy subdivided octahedral sphere of profiles/mesh_decimate.json and on the same sphere without "
                    "the faces whose centroid has z > 0.8, fp32 vertices, one MI355X; borders='fixed' and borders='collapse' alternating "
                    "in one process, wall clock around a device synchronisation, median of 20 after 3 warm-up calls each",
            "device": torch.cuda.get_device_name(dev), "rows": rows}


def quality():
    import _decimate_ref as R
    from actionmesh_amd import mesh_decimate as MD
    rows = []
    for name, (v, f), target in (("icosphere3", R.icosphere(3), 200), ("torus32x16", R.torus(32, 16), 160),
                                 ("jittered4", R.jittered_icosphere(4), 512)):
        nv, nf, rounds = MD.decimate_mesh(torch.from_numpy(v), torch.from_numpy(f), target, backend=R.NumpyBackend(), return_rounds=True)
        nv, nf = nv.numpy(), nf.numpy()
        t0 = time.perf_counter()
        gv, gf = R.greedy_decimate(v, f, nf.shape[0])
        greedy_s = time.perf_counter() - t0
        ours, theirs = R.surface_distance(v, f, nv, nf), R.surface_distance(v, f, gv, gf)
        rows.append({"mesh": name, "faces": int(f.shape[0]), "faces_after": int(nf.shape[0]), "rounds": rounds,
                     "round_scheme_distance": ours, "sequential_greedy_distance": theirs, "ratio": round(ours / theirs, 4),
                     "sequential_greedy_numpy_restatement_seconds": round(greedy_s, 1)})
        print(json.dumps(rows[-1]))
    return {"what": "symmetric mean nearest-neighbour distance between 20 000 area-uniform samples of the original surface and of the "
                    "result (fixed seeds), round scheme over a sequential greedy decimation with the same cost and validity rules at "
                    "the same face count; both through the numpy restatement of tests/_decimate_ref.py, on the CPU",
            "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/mesh_decimate.json, with --borders collapse profiles/mesh_decimate_borders.json")
    ap.add_argument("--subdivisions", type=int, nargs="+", default=[224, 112])
    ap.add_argument("--target", type=int, default=40000)
    ap.add_argument("--quality", action="store_true", help="only re-measure the quality ratios (no GPU)")
    ap.add_argument("--borders", choices=("fixed", "collapse"), default="fixed",
                    help="collapse: time borders='collapse' against 'fixed' on the closed sphere and on the sphere with one cap cut off")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "mesh_decimate_borders.json" if a.borders == "collapse" else "mesh_decimate.json")
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            out = json.load(fh)
    if a.quality:
        out["quality"] = quality()
    elif a.borders == "collapse":
        out["timing"] = border_timing(a.subdivisions[0], a.target, torch.device("cuda:0"))
    else:
        from actionmesh_amd import mesh_decimate as MD
        dev = torch.device("cuda:0")
        rows = []
        for n in a.subdivisions:
            v, f = noisy_sphere(n)
            verts, faces = torch.from_numpy(v).float().to(dev), torch.from_numpy(f).to(dev)
            nv, nf, rounds = MD.decimate_mesh(verts, faces, a.target, return_rounds=True)
            t = timed(lambda: MD.decimate_mesh(verts, faces, a.target), 20, 3, dev)
            rows.append({"subdivisions": n, "vertices": int(v.shape[0]), "faces": int(f.shape[0]), "target_faces": a.target,
                         "faces_after": int(nf.shape[0]), "vertices_after": int(nv.shape[0]), "rounds": rounds, "decimate_mesh": t,
                         "ms_per_round": round(t["median_ms"] / max(rounds, 1), 3)})
            print(json.dumps(rows[-1]))
        out["timing"] = {"what": "decimate_mesh on a noisy subdivided octahedral sphere, fp32 vertices, one MI355X; wall clock around a "
                                 "device synchronisation, median of 20 after 3 warm-up calls",
                         "comparison": "none with fast_simplification (not installable offline)",
                         "device": torch.cuda.get_device_name(dev), "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
