"""`decimate_mesh(..., borders="collapse")` on CPU tensors, through the numpy restatement of the header's "Border collapses"
(tests/_decimate_border_ref.py) as its backend: open meshes reach the target with the open-manifold invariants, the flat grid stays
exactly flat inside its exact outline, closed meshes come out with the bits of `borders="fixed"`, the cases of the topology rule, the
independence of one round's selection, the quality against a sequential greedy decimation with the same rules
(profiles/mesh_decimate_borders.json) and the arguments."""
import json
import logging
import os

import numpy as np
import pytest
import torch

import _decimate_border_ref as B
import _decimate_ref as R
from actionmesh_amd import mesh_decimate as MD
from actionmesh_amd import mesh_prep as MP

BACKEND = B.NumpyBorderBackend()
OPEN = {"grid12": (lambda: R.grid(12), 40), "half_icosphere3": (lambda: B.half_icosphere(3), 60),
        "cylinder16x8": (lambda: B.open_cylinder(16, 8), 64)}
# parallel / sequential greedy at the same face count: (surface distance ratio, border curve distance ratio), measured with this file
# (`measure_quality`; profiles/mesh_decimate_borders.json has the distances).  The runs are bit-reproducible: the margin of 1.25 only
# absorbs a later change of the sample seeds.  None is above 1.5.  The flat grid's border curve is kept exactly - both distances are
# rounding noise around 1e-17 - so there the curve is held to 1e-12 instead of to a ratio of two roundings.
QUALITY = {"grid12": (0.9904, None), "half_icosphere3": (0.9886, 0.8992), "cylinder16x8": (1.0024, 0.9788)}
_runs = {}


def collapse(v, f, target, **kw):
    return MD.decimate_mesh(torch.from_numpy(v), torch.from_numpy(f), target, backend=BACKEND, borders="collapse", **kw)


def run(name):
    """One `borders="collapse"` run per open mesh, shared and left unchanged: (v, f, (vertices', faces', map, rounds))."""
    if name not in _runs:
        make, target = OPEN[name]
        v, f = make()
        _runs[name] = (v, f, collapse(v, f, target, return_map=True, return_rounds=True))
    return _runs[name]


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("name", list(OPEN))
def test_open_meshes_reach_the_target_with_the_invariants(name):
    v, f, (nv, nf, vmap, rounds) = run(name)
    target = OPEN[name][1]
    assert nf.shape[0] in (target, target - 1) and rounds > 0
    B.check_open_manifold(nv.numpy(), nf.numpy(), R.euler(v.shape[0], f), len(B.border_loops(f)), B.components(f))
    assert torch.equal(vmap[vmap], vmap)
    again = collapse(v, f, target, return_map=True, return_rounds=True)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(again[:3], (nv, nf, vmap))) and again[3] == rounds
    v32, f32 = collapse(v.astype(np.float32), f.astype(np.int32), target)
    assert v32.dtype == torch.float32 and f32.dtype == torch.int32 and f32.shape[0] in (target, target - 1)


def test_the_flat_grid_stays_flat_inside_its_exact_outline():
    """Every collapse the restatement applies down to 40 faces has cost exactly 0 (checked here, every round), so the target of 40
    stands as it is: the surface stays in z = 0, the border on the square's outline, the corners where they were."""
    v, f = R.grid(12)
    kept_costs = []
    pos, faces, _, _ = MD.decimate_rounds(torch.from_numpy(v), torch.from_numpy(f.astype(np.int32)), 40, backend=BACKEND, borders="collapse",
                                          observer=lambda r, s: kept_costs.append(s["cost"][s["kept"]].clone()))
    assert len(kept_costs) > 1 and all((c == 0.0).all() for c in kept_costs)
    nv, nf = B._compact(pos.numpy(), faces.numpy().astype(np.int64))
    assert nf.shape[0] in (40, 39) and (nv[:, 2] == 0).all()
    on_border = np.unique(np.concatenate(B.border_loops(nf)))
    assert (np.isin(nv[on_border, :2], (0.0, 11.0)).any(1)).all()
    for corner in ((0, 0, 0), (0, 11, 0), (11, 0, 0), (11, 11, 0)):
        assert (nv == np.array(corner, dtype=np.float64)).all(1).any()
    areas = R.face_areas(nv, nf)
    assert abs(areas.sum() - 121.0) <= 1e-12 and (areas > 0).all()


@pytest.mark.parametrize("name, make, target", [("icosphere3", lambda: R.icosphere(3), 200), ("torus32x16", lambda: R.torus(32, 16), 160)])
def test_closed_meshes_equal_the_fixed_mode_bit_for_bit(name, make, target):
    v, f = make()
    got = collapse(v, f, target, return_map=True, return_rounds=True)
    want = MD.decimate_mesh(torch.from_numpy(v), torch.from_numpy(f), target, backend=BACKEND, return_map=True, return_rounds=True)
    assert got[3] == want[3] and all(torch.equal(bits(a), bits(b)) for a, b in zip(got[:3], want[:3]))


@pytest.mark.parametrize("name", ["isolated triangle", "strip"])
def test_meshes_without_a_permitted_collapse_come_back_whole(name, caplog):
    v, f = B.isolated_triangle() if name == "isolated triangle" else B.strip()
    with caplog.at_level(logging.WARNING, logger="actionmesh_amd.mesh_decimate"):
        nv, nf = collapse(v, f, 0)
    assert "no edge can collapse" in caplog.text
    assert np.array_equal(nv.numpy(), v) and np.array_equal(nf.numpy(), f)


def test_a_hole_of_three_edges_stays_and_a_hole_of_four_may_shrink_to_three():
    v, f = B.holes_grid(7)
    assert sorted(len(loop) for loop in B.border_loops(f)) == [3, 4, 24]
    nv, nf = collapse(v, f, 20)
    B.check_open_manifold(nv.numpy(), nf.numpy(), R.euler(v.shape[0], f), 3)
    outer, *holes = sorted((len(loop) for loop in B.border_loops(nf.numpy())), reverse=True)
    assert nf.shape[0] in (20, 19) and sorted(holes) in ([3, 3], [3, 4])


def test_the_ear_disappears():
    v, f, ear = B.ear_disc()
    """Both border edges of the ear are candidates from the first round on; they cost more than the flat disc's collapses, which cost
    nothing, so the ear goes once those are used up."""
    faces = f.astype(np.int32)
    tables = R.np_topology(faces, v.shape[0]) + R.np_edges(faces, v.shape[0])
    Q = B.ref_border_quadrics(v, faces, tables[0], tables[1], tables[3], tables[4])
    _, cost, key = B.ref_border_edges(v, Q, faces, *tables)
    at_ear = (tables[2] == ear).any(1)
    assert at_ear.sum() == 2 and (key[at_ear] != B.NO_KEY).all() and (cost[at_ear] > 0).all()
    nv, nf, vmap = collapse(v, f, 3, return_map=True)
    assert nf.shape[0] in (3, 2) and vmap[ear] != ear and not (nv.numpy() == v[ear]).all(1).any()
    B.check_open_manifold(nv.numpy(), nf.numpy(), 1, 1)


def test_locked_vertices_stay_where_they_are():
    v, f, shared = B.bow_tie()
    nv, nf, vmap = collapse(v, f, 4, return_map=True)
    assert nf.shape[0] < f.shape[0] and vmap[shared] == shared and (vmap == shared).sum() == 1
    assert (nv.numpy() == v[shared]).all(1).any()
    v, f, (a, b) = R.finned_sphere()
    nv, nf, vmap = collapse(v, f, 100, return_map=True)
    assert nf.shape[0] < f.shape[0]
    for s in (a, b):
        assert vmap[s] == s and (vmap == s).sum() == 1 and (nv.numpy() == v[s]).all(1).any()


@pytest.mark.parametrize("name", ["half_icosphere3", "holes"])
def test_an_interior_edge_between_two_border_vertices_is_never_selected(name):
    v, f = B.half_icosphere(3) if name == "half_icosphere3" else B.holes_grid(7)
    seen = []

    def observer(r, s):
        edges, count = s["tables"].edges.numpy(), s["tables"].edge_count.numpy()
        cls = B.vertex_classes(v.shape[0], edges, count)
        pinch = (count == 2) & (cls[edges[:, 0]] != B.INTERIOR) & (cls[edges[:, 1]] != B.INTERIOR)
        seen.append(int(pinch.sum()))
        assert not (s["selected"].numpy()[pinch]).any() and (s["key"].numpy()[pinch] == B.NO_KEY).all()

    MD.decimate_rounds(torch.from_numpy(v), torch.from_numpy(f.astype(np.int32)), 20, backend=BACKEND, borders="collapse", observer=observer)
    assert len(seen) > 1 and max(seen) > 0


def test_the_closed_stars_of_one_selection_are_disjoint():
    v, f = B.half_icosphere(3)
    first = {}
    MD.decimate_rounds(torch.from_numpy(v), torch.from_numpy(f.astype(np.int32)), 600, backend=BACKEND, borders="collapse",
                       observer=lambda r, s: first.setdefault("s", {k: s[k] for k in ("selected", "tables", "faces")}))
    s = first["s"]
    edges, faces = s["tables"].edges.numpy(), s["faces"].numpy()
    chosen = edges[s["selected"].numpy() != 0]
    count = s["tables"].edge_count.numpy()[s["selected"].numpy() != 0]
    assert chosen.shape[0] > 4 and (count == 1).any() and (count == 2).any()
    owner = np.full(faces.shape[0], -1)
    for i, (a, b) in enumerate(chosen):
        star = np.isin(faces, (a, b)).any(1)
        assert (owner[star] == -1).all()
        owner[star] = i


def measure_quality(name):
    """(surface distance, greedy's, border curve distance, greedy's) to the original, at the parallel result's face count."""
    v, f, (nv, nf, _, _) = run(name)
    nv, nf = nv.numpy(), nf.numpy()
    gv, gf = B.greedy_border_decimate(v, f, nf.shape[0])
    assert gf.shape[0] in (nf.shape[0], nf.shape[0] - 1)
    return (R.surface_distance(v, f, nv, nf), R.surface_distance(v, f, gv, gf), B.border_curve_distance(v, f, nv, nf),
            B.border_curve_distance(v, f, gv, gf))


@pytest.mark.parametrize("name", list(OPEN))
def test_quality_against_the_sequential_greedy_decimation(name):
    surface, greedy_surface, curve, greedy_curve = measure_quality(name)
    want_surface, want_curve = QUALITY[name]
    print(f"{name}: surface {surface:.6g} / {greedy_surface:.6g} = {surface / greedy_surface:.4f}, border curve {curve:.6g} / {greedy_curve:.6g}")
    assert want_surface <= 1.5 and surface / greedy_surface <= want_surface * 1.25
    if want_curve is None:
        assert curve <= 1e-12 and greedy_curve <= 1e-12
    else:
        assert want_curve <= 1.5 and curve / greedy_curve <= want_curve * 1.25
    with open(os.path.join(os.path.dirname(__file__), "..", "profiles", "mesh_decimate_borders.json")) as fh:
        recorded = json.load(fh)["quality_cpu"][name]
    assert abs(recorded["surface_ratio"] - want_surface) < 1e-3
    assert recorded["border_curve_ratio"] is None if want_curve is None else abs(recorded["border_curve_ratio"] - want_curve) < 1e-3


def test_bad_arguments_raise():
    v, f = (torch.from_numpy(a) for a in R.grid(4))
    for bad in ("move", None, "Collapse", 1):
        with pytest.raises(ValueError, match="borders"):
            MD.decimate_mesh(v, f, 4, backend=BACKEND, borders=bad)
    for bad in (-1.0, float("nan"), float("inf"), "heavy"):
        with pytest.raises(ValueError, match="border_weight"):
            MD.decimate_mesh(v, f, 4, backend=BACKEND, borders="collapse", border_weight=bad)
        with pytest.raises(ValueError, match="border_weight"):
            MD.decimate_rounds(v, f.to(torch.int32), 4, backend=BACKEND, border_weight=bad)
    with pytest.raises(ValueError, match="decimate_borders"):
        MP.process_mesh(v, f, face_decimation=4, decimation="hip", decimate_borders="move")


def test_a_border_weight_of_zero_still_reaches_the_target():
    v, f = B.half_icosphere(3)
    nv, nf = collapse(v, f, 60, border_weight=0)
    assert nf.shape[0] in (60, 59)
    B.check_open_manifold(nv.numpy(), nf.numpy(), 1, 1)


def test_process_mesh_passes_the_keyword_through(monkeypatch):
    calls = []

    def recorder(vertices, faces, target_faces, **kw):
        calls.append(kw)
        return MD_decimate(vertices, faces, target_faces, backend=BACKEND, **kw)

    MD_decimate = MD.decimate_mesh
    monkeypatch.setattr(MD, "decimate_mesh", recorder)
    v, f = R.grid(12)
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    _, fixed = MP.process_mesh(tv, tf, face_decimation=40, decimation="hip")
    _, moved = MP.process_mesh(tv, tf, face_decimation=40, decimation="hip", decimate_borders="collapse")
    assert [c.get("borders", "fixed") for c in calls] == ["fixed", "collapse"]
    assert fixed.shape[0] == 100 and moved.shape[0] in (40, 39)            # today's stop on this grid, and the target
