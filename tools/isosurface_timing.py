#!/usr/bin/env python
"""Times the iso-surface extraction (actionmesh_amd/isosurface.py over csrc/am_isosurface.hip) on one MI355X, on a sphere field and a
gyroid-like field (many sheets: about six times the sphere's triangles) sampled on 257^3 and 513^3 points - the two grids of the
reference's Stage-0 call.  Per field and grid:

  * each kernel by HIP events around its launch (median of 20 after 3 warm-up launches), the tables prepared once; for am_iso_classify
    also the achieved GB/s against the 6 bytes per point the pass has to move (4 read, 2 written);
  * the whole `extract_isosurface` call, wall clock around a device synchronisation (the same median): the kernels, the popcount
    gather, the two int64 prefix sums, the two device-to-host reads and the compaction of unused vertices;
and once: `hierarchical_extract_geometry` 8 -> 9 with the analytic sphere evaluated on the device (median of 5 after 1 warm-up call),
with the share of the 513^3 fine points it evaluated.

`diso` and skimage are not installable offline, so there is no figure of either here.  The only host figure is the tests' own NUMPY
RESTATEMENT of the contract (tests/_isosurface_ref.py) at 65^3 on the same box - a yardstick the tests compare bits with, not an
implementation anyone would ship, and labelled as that in the output.

Writes profiles/isosurface.json; no test asserts a time.

`--method dual` measures the second extraction (dual marching cubes, csrc/am_dualcubes.hip) against the first IN ONE PROCESS: per field
and grid the four am_dmc_* kernels by HIP events, then the whole `extract_isosurface` call of both methods, alternating call by call
(wall clock around a device synchronisation), and - what the method is for - `merge_and_clean_mesh` + `decimate_mesh` of the 257^3
sphere mesh of either method to 40 000 faces: rounds and milliseconds, alternating too.  Writes profiles/isosurface_dual.json.

    python tools/isosurface_timing.py [--method tetrahedra|dual] [--out profiles/isosurface.json] [--grids 257 513]
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

BOUNDS = (-1.005,) * 3 + (1.005,) * 3


def sphere_of(points):
    x, y, z = points[..., 0], points[..., 1], points[..., 2]
    return 0.8 - torch.sqrt((x - 0.03) ** 2 + (y + 0.02) ** 2 + (z - 0.01) ** 2)


def gyroid_of(points, cells=4.0):
    x, y, z = (points[..., c] * (cells * np.pi) for c in range(3))
    return torch.sin(x) * torch.cos(y) + torch.sin(y) * torch.cos(z) + torch.sin(z) * torch.cos(x)


def grid_field(fn, n, dev):
    axis = torch.from_numpy(np.linspace(-1.005, 1.005, n).astype(np.float32)).to(dev)
    out = torch.empty((n, n, n), dtype=torch.float32, device=dev)
    for i in range(n):                                              # slab by slab: no (n^3, 3) point array
        out[i] = fn(torch.stack(torch.meshgrid(axis[i:i + 1], axis, axis, indexing="ij"), dim=-1))[0]
    return out


def summary(times):
    return {"median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4), "n": len(times)}


def by_events(fn, repeats, warmup, dev):
    times = []
    for k in range(warmup + repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize(dev)
        if k >= warmup:
            times.append(start.elapsed_time(end))
    return summary(times)


def by_clock(fn, repeats, warmup, dev):
    times = []
    for k in range(warmup + repeats):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        if k >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return summary(times)


def alternating(fns, repeats, warmup, dev):
    """by_clock for several callables, one call of each per round, so that drift of the clocks or of the box hits all alike."""
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


def main_dual(a):
    from actionmesh_amd import isosurface as ISO
    from actionmesh_amd import mesh_decimate, mesh_prep, ops
    dev = torch.device("cuda:0")
    rows = []
    for name, fn in (("sphere", sphere_of), ("gyroid", gyroid_of)):
        for n in a.grids:
            values = grid_field(fn, n, dev)
            config, double = ops.dmc_cells(values)
            code, count, edge_mask = ops.dmc_classify(config, double)
            triangles = 2 * torch.tensor(ISO._POPCOUNT[:8], dtype=torch.int64, device=dev)[edge_mask.reshape(-1).long()]
            vertex_end, tri_end = torch.cumsum(count.reshape(-1), 0, dtype=torch.int64), torch.cumsum(triangles, 0)
            V, F = int(vertex_end[-1]), int(tri_end[-1])
            voff, toff = (vertex_end - count.reshape(-1)).view(values.shape), (tri_end - triangles).view(values.shape)
            flipped = int((code >> 8).sum()) // 2
            del triangles, vertex_end, tri_end
            vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
            faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
            flag = torch.zeros((1,), dtype=torch.int32, device=dev)
            origin, spacing = BOUNDS[:3], ((BOUNDS[3] - BOUNDS[0]) / (n - 1),) * 3
            t_cells = by_events(lambda: ops.dmc_cells(values, out_config=config, out_double=double), 20, 3, dev)
            t_classify = by_events(lambda: ops.dmc_classify(config, double, out_code=code, out_count=count, out_edge_mask=edge_mask), 20, 3, dev)
            t_vertices = by_events(lambda: ops.dmc_vertices(values, code, voff, V, origin, spacing, out=vertices, flag=flag), 20, 3, dev)
            bad = int(flag)
            t_triangles = by_events(lambda: ops.dmc_triangles(code, edge_mask, voff, toff, vertices, V, F, out=faces, flag=flag), 20, 3, dev)
            assert bad == 0 and int(flag) == 0
            del voff, toff, vertices, faces, config, double, code, count, edge_mask
            whole = alternating({"tetrahedra": lambda: ISO.extract_isosurface(values, bounds=BOUNDS),
                                 "dual": lambda: ISO.extract_isosurface(values, bounds=BOUNDS, method="dual")}, 20, 3, dev)
            tet_faces = int(ISO.extract_isosurface(values, bounds=BOUNDS)[1].shape[0])
            rows.append({"field": name, "grid": n, "points": n ** 3, "dual_vertices_before_compaction": V, "dual_triangles": F,
                         "flipped_faces": flipped, "tetrahedra_triangles": tet_faces, "triangle_ratio": round(F / tet_faces, 4),
                         "am_dmc_cells": t_cells, "am_dmc_cells_GBps_at_6_bytes_per_point": round(6 * n ** 3 / t_cells["median_ms"] / 1e6, 1),
                         "am_dmc_classify": t_classify, "am_dmc_vertices": t_vertices, "am_dmc_triangles": t_triangles,
                         "extract_isosurface": whole})
            print(json.dumps(rows[-1]), flush=True)
            del values
    values = grid_field(sphere_of, a.decimate_grid, dev)
    meshes, rounds = {}, {}
    for method in ISO.METHODS:
        v, f = ISO.extract_isosurface(values, bounds=BOUNDS, method=method)
        meshes[method] = mesh_prep.merge_and_clean_mesh(v, f)[:2]

    def decimate(method):
        dv, df, rounds[method] = mesh_decimate.decimate_mesh(*meshes[method], a.decimate_faces, return_rounds=True)
        assert df.shape[0] == a.decimate_faces

    t_decimate = alternating({m: (lambda m=m: decimate(m)) for m in ISO.METHODS}, 5, 1, dev)
    decimation = {"field": "sphere", "grid": a.decimate_grid, "target_faces": a.decimate_faces,
                  **{m: {"faces_in": int(meshes[m][1].shape[0]), "rounds": rounds[m], "decimate_mesh": t_decimate[m]} for m in ISO.METHODS}}
    print(json.dumps(decimation), flush=True)
    out = {"what": "iso-surface extraction by dual marching cubes against marching tetrahedra on one MI355X, one process: kernels by HIP "
                   "events (medians of 20 after 3 warm-up launches), whole calls by wall clock around a device synchronisation, the two "
                   "methods alternating call by call (medians of 20 after 3; the decimation: 5 after 1)",
           "comparison": "none with diso or skimage (not installable offline)",
           "device": torch.cuda.get_device_name(dev), "rows": rows, "decimation": decimation}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--method", choices=["tetrahedra", "dual"], default="tetrahedra")
    ap.add_argument("--out", default=None, help="default: profiles/isosurface.json, or profiles/isosurface_dual.json with --method dual")
    ap.add_argument("--decimate-grid", type=int, default=257)
    ap.add_argument("--decimate-faces", type=int, default=40_000)
    ap.add_argument("--grids", type=int, nargs="+", default=[257, 513])
    ap.add_argument("--hierarchy", type=int, nargs=2, default=[8, 9], metavar=("DENSE", "FINEST"))
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "isosurface_dual.json" if a.method == "dual" else "isosurface.json")
    if a.method == "dual":
        return main_dual(a)
    from actionmesh_amd import isosurface as ISO
    from actionmesh_amd import ops
    import _isosurface_ref as R
    dev = torch.device("cuda:0")
    rows = []
    for name, fn in (("sphere", sphere_of), ("gyroid", gyroid_of)):
        for n in a.grids:
            values = grid_field(fn, n, dev)
            mask, count = ops.iso_classify(values)
            crossings = torch.tensor(ISO._POPCOUNT, dtype=torch.int64, device=dev)[mask.reshape(-1).long()]
            vertex_end, tri_end = torch.cumsum(crossings, 0), torch.cumsum(count.reshape(-1), 0, dtype=torch.int64)
            V, F = int(vertex_end[-1]), int(tri_end[-1])
            voff, toff = (vertex_end - crossings).view(values.shape), (tri_end - count.reshape(-1)).view(values.shape)
            del crossings, vertex_end, tri_end
            vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
            faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
            flag = torch.zeros((1,), dtype=torch.int32, device=dev)
            origin, spacing = BOUNDS[:3], ((BOUNDS[3] - BOUNDS[0]) / (n - 1),) * 3
            t_classify = by_events(lambda: ops.iso_classify(values, out_mask=mask, out_count=count), 20, 3, dev)
            t_vertices = by_events(lambda: ops.iso_vertices(values, mask, voff, V, origin, spacing, out=vertices, flag=flag), 20, 3, dev)
            t_triangles = by_events(lambda: ops.iso_triangles(values, mask, count, voff, toff, V, F, out=faces, flag=flag), 20, 3, dev)
            assert int(flag) == 0
            del voff, toff, vertices, faces
            t_whole = by_clock(lambda: ISO.extract_isosurface(values, bounds=BOUNDS), 20, 3, dev)
            rows.append({"field": name, "grid": n, "points": n ** 3, "vertices": V, "triangles": F,
                         "am_iso_classify": t_classify, "am_iso_classify_GBps_at_6_bytes_per_point": round(6 * n ** 3 / t_classify["median_ms"] / 1e6, 1),
                         "am_iso_vertices": t_vertices, "am_iso_triangles": t_triangles, "extract_isosurface": t_whole})
            print(json.dumps(rows[-1]), flush=True)
            del values, mask, count
    evaluated = []

    def field(points):
        evaluated.append(points.shape[1])
        return sphere_of(points).unsqueeze(-1)

    dense, finest = a.hierarchy
    t_hier = by_clock(lambda: ISO.hierarchical_extract_geometry(field, dev, bounds=BOUNDS, dense_octree_depth=dense,
                                                                hierarchical_octree_depth=finest), 5, 1, dev)
    per_call = sum(evaluated) // 6
    fine = per_call - (2 ** dense + 1) ** 3 if finest == dense + 1 else None
    hierarchy = {"field": "sphere, evaluated on the device inside the timed call", "dense_octree_depth": dense, "hierarchical_octree_depth": finest,
                 "dilation": 1, "points_evaluated_per_call": per_call, "fine_points_evaluated": fine,
                 "fine_points_share": None if fine is None else round(fine / (2 ** finest + 1) ** 3, 4),
                 "hierarchical_extract_geometry": t_hier}
    print(json.dumps(hierarchy), flush=True)
    x = np.linspace(-1.005, 1.005, 65)
    gx, gy, gz = np.meshgrid(x, x, x, indexing="ij")
    host_values = R.sphere_of(gx, gy, gz).astype(np.float32)
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        hv, hf = R.ref_extract(host_values, 0.0, BOUNDS[:3], ((BOUNDS[3] - BOUNDS[0]) / 64,) * 3)
        host.append((time.perf_counter() - t0) * 1e3)
    out = {"what": "iso-surface extraction (marching tetrahedra) on one MI355X: kernels by HIP events, whole calls by wall clock around a "
                   "device synchronisation; medians of 20 after 3 warm-up runs (the hierarchy: 5 after 1)",
           "comparison": "none with diso or skimage (not installable offline)",
           "device": torch.cuda.get_device_name(dev), "rows": rows, "hierarchy": hierarchy,
           "numpy_restatement_of_the_contract_65_cubed_on_the_host": {"what": "tests/_isosurface_ref.py ref_extract, the yardstick of the tests - a "
                                                                      "restatement, not an implementation", "triangles": int(hf.shape[0]),
                                                                      "ms": summary(host)}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
