#!/usr/bin/env python
"""Times the anchor-mesh preparation (actionmesh_amd/mesh_prep.py over csrc/am_mesh.hip) on one MI355X, and beside each number the
numpy restatement the tests compare it with, on the same box and in the same process.  The restatement is NOT trimesh (which is not
installable offline): it is the header's contract written in numpy fp64 (tests/test_mesh_prep_gpu.py), and for the clean-up the same
torch plumbing on CPU tensors.

    get_mesh_features(with_normals)   one frame, fp32 vertices, topology built once (as VertexFeatures keeps it)
    merge_and_clean_mesh              the dirty torus of tools/e2e_synthetic.py (duplicated seam, degenerate and duplicate faces), fp64
    sample_surface(16384)             areas + prefix sum + host draws + upload + samples

at V = 50 000 and V = 400 000 (F = 2 V).  Wall clock around a device synchronisation, median of 20 after 3 warm-up calls (host
restatements: median of 5).  Writes profiles/mesh_prep.json; no test asserts a time.

    python tools/mesh_prep_timing.py [--out profiles/mesh_prep.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, repeats, warmup, dev=None):
    times = []
    for k in range(warmup + repeats):
        if dev is not None:
            torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        if dev is not None:
            torch.cuda.synchronize(dev)
        if k >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(times), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3), "n": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_prep.json"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[50000, 400000])
    a = ap.parse_args()
    import e2e_synthetic as E
    import test_mesh_prep_gpu as tg                 # the numpy restatements
    from actionmesh_amd import mesh_prep as MP
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    rows = []
    for V in a.sizes:
        v, f, cols = E.torus_mesh(V)
        dv, df = E.dirty_mesh(v, f, cols)
        v32 = torch.from_numpy(v).float()
        verts, faces = v32.to(dev), torch.from_numpy(f).to(dev)
        features = MP.VertexFeatures(faces)
        widened = v32.double().numpy()
        raw_v, raw_f = torch.from_numpy(dv), torch.from_numpy(df)
        dev_v, dev_f = raw_v.to(dev), raw_f.to(dev)

        def host_samples():
            u_face, u_bary = MP.draw_uniforms(16384, 0)
            tg.ref_samples(widened, f, np.cumsum(tg.ref_faces(widened, f)[2] / 2.0), u_face, u_bary)
        rows.append({
            "vertices": V, "faces": int(len(f)), "dirty_vertices": int(len(dv)), "dirty_faces": int(len(df)),
            "get_mesh_features": {"device": timed(lambda: features(verts), 20, 3, dev),
                                  "topology_build_once": timed(lambda: MP.MeshTopology(faces, V), 20, 3, dev),
                                  "numpy_restatement": timed(lambda: tg.ref_normals(widened, f), 5, 1)},
            "merge_and_clean_mesh": {"device": timed(lambda: MP.merge_and_clean_mesh(dev_v, dev_f), 20, 3, dev),
                                     "same_call_on_cpu_tensors": timed(lambda: MP.merge_and_clean_mesh(raw_v, raw_f), 5, 1)},
            "sample_surface_16384": {"device": timed(lambda: MP.sample_surface(verts, faces, 16384, seed=0), 20, 3, dev),
                                     "numpy_restatement": timed(host_samples, 5, 1)},
        })
        print(json.dumps(rows[-1]))
    out = {"what": "anchor-mesh preparation, one MI355X; wall clock around a device synchronisation, median of 20 after warm-up "
                   "(host: median of 5)",
           "comparison": "numpy restatement, not trimesh (the contract of include/actionmesh_amd.h in numpy fp64, as the tests use it); "
                         "merge_and_clean_mesh: the same torch plumbing on CPU tensors",
           "device": torch.cuda.get_device_name(dev), "host_threads": torch.get_num_threads(), "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
