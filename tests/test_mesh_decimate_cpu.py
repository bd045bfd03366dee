"""Mesh decimation without a GPU: the round loop of actionmesh_amd/mesh_decimate.py on CPU tensors, driven through a numpy fp64
restatement of the four kernels written from the header's text (tests/_decimate_ref.py).  Invariants on every mesh, the refusals
and edge cases, the independence of a round's selection, the round count as a condition (a tie-break by raw edge index needs
hundreds of rounds on regular meshes), the surface distance against a sequential greedy decimation, and process_mesh's keyword."""
import logging

import numpy as np
import pytest
import torch

import _decimate_ref as R
from actionmesh_amd import mesh_decimate as MD
from actionmesh_amd import mesh_prep as MP

BACKEND = R.NumpyBackend()
MESHES = {"icosphere3": (lambda: R.icosphere(3), 200), "torus32x16": (lambda: R.torus(32, 16), 160),
          "jittered4": (lambda: R.jittered_icosphere(4), 512)}
# symmetric mean nearest-neighbour distance of the round scheme over that of the sequential greedy decimation at the same face count,
# measured on the CPU with the restatement (profiles/mesh_decimate.json, "quality").  The runs are bit-reproducible: the 25 % only
# absorb a later change of the sample seeds.  None is above 1.5.
MEASURED_RATIO = {"icosphere3": 0.9938, "torus32x16": 1.0268, "jittered4": 0.9939}


def run(v, f, target, **kw):
    out = MD.decimate_mesh(torch.from_numpy(v), torch.from_numpy(f), target, backend=BACKEND, **kw)
    return tuple(t.numpy() if isinstance(t, torch.Tensor) else t for t in out)


@pytest.fixture(scope="module")
def results():
    """name -> dict(v, f, target, nv, nf, map, rounds, first: the state after the first round's selection)."""
    out = {}
    for name, (make, target) in MESHES.items():
        v, f = make()
        first = {}

        def observer(r, state, first=first):
            if r == 0:
                first.update({k: (t.clone() if isinstance(t, torch.Tensor) else t) for k, t in state.items()})

        pos, live, merged, rounds = MD.decimate_rounds(torch.from_numpy(v), torch.from_numpy(f).to(torch.int32), target, backend=BACKEND,
                                                       observer=observer)
        nv, nf, vmap, rounds2 = run(v, f, target, return_map=True, return_rounds=True)
        assert rounds == rounds2
        out[name] = dict(v=v, f=f, target=target, nv=nv, nf=nf, map=vmap, rounds=rounds, first=first, positions=pos.numpy())
    return out


@pytest.mark.parametrize("name", list(MESHES))
def test_invariants(results, name):
    r = results[name]
    v, f, nv, nf, vmap = r["v"], r["f"], r["nv"], r["nf"], r["map"]
    assert nf.shape[0] in (r["target"], r["target"] - 1)
    assert nv.dtype == v.dtype and nf.dtype == f.dtype and vmap.dtype == np.int64 and vmap.shape == (v.shape[0],)
    R.check_closed_manifold(nv, nf, R.euler(v.shape[0], f))
    assert np.array_equal(vmap[vmap], vmap)
    fixed = np.nonzero(vmap == np.arange(v.shape[0]))[0]
    assert fixed.shape[0] == nv.shape[0] and np.array_equal(r["positions"][fixed].view(np.int64), nv.view(np.int64))
    again = run(v, f, r["target"], return_map=True)
    assert all(np.array_equal(a, b) for a, b in zip(again, (nv, nf, vmap))) and np.array_equal(again[0].view(np.int64), nv.view(np.int64))


@pytest.mark.parametrize("name", list(MESHES))
def test_first_selection_is_independent(results, name):
    """The closed face stars of the edges selected in the first round are pairwise disjoint."""
    s = results[name]["first"]
    faces, edges = s["faces"].numpy(), s["tables"].edges.numpy()
    chosen = edges[s["selected"].numpy() != 0]
    assert chosen.shape[0] > 1
    owner = np.full(faces.shape[0], -1)
    for i, (u, v) in enumerate(chosen):
        star = np.nonzero((faces == u).any(1) | (faces == v).any(1))[0]
        assert (owner[star] == -1).all(), (i, owner[star])
        owner[star] = i


def test_round_count(results):
    """The prototype needed 56 rounds on a torus and 33 on an icosphere; an unhashed tie-break needs hundreds."""
    assert results["torus32x16"]["rounds"] <= 100 and results["icosphere3"]["rounds"] <= 100, {k: r["rounds"] for k, r in results.items()}


def test_float32_input_keeps_dtype_and_unmoved_bits(results):
    r = results["icosphere3"]
    v32 = r["v"].astype(np.float32)
    nv, nf, vmap = run(v32, r["f"].astype(np.int32), r["target"], return_map=True)
    assert nv.dtype == np.float32 and nf.dtype == np.int32
    R.check_closed_manifold(nv.astype(np.float64), nf, 2)


def test_at_or_below_target_is_returned_as_it_is():
    v, f = R.icosphere(1)
    tv, tf = torch.from_numpy(v).float(), torch.from_numpy(f)
    for target in (f.shape[0], f.shape[0] + 7):
        nv, nf, vmap = MD.decimate_mesh(tv, tf, target, return_map=True, backend=BACKEND)
        assert nv is tv and nf is tf and torch.equal(vmap, torch.arange(v.shape[0]))
    assert MD.decimate_mesh(tv, tf)[0] is tv                                     # the reference's default of 40 000


@pytest.mark.parametrize("make", [R.glued_tetrahedra, R.tetrahedron], ids=["glued", "tetrahedron"])
def test_unreachable_target_ends_without_raising(make, caplog):
    v, f = make()
    with caplog.at_level(logging.WARNING, logger=MD.logger.name):
        nv, nf = run(v, f, 2)
    assert np.array_equal(nv, v) and np.array_equal(nf, f)
    assert any("no edge can collapse" in rec.getMessage() for rec in caplog.records)


def test_open_grid_keeps_border_plane_and_area():
    v, f = R.grid(12)
    nv, nf, vmap = run(v, f, 100, return_map=True)
    assert nf.shape[0] < f.shape[0]
    i, j = np.divmod(np.arange(144), 12)
    border = np.nonzero((i == 0) | (i == 11) | (j == 0) | (j == 11))[0]
    assert np.array_equal(vmap[border], border)
    fixed = np.nonzero(vmap == np.arange(144))[0]
    where = {int(o): n for n, o in enumerate(fixed)}
    assert all(np.array_equal(nv[where[int(b)]], v[b]) for b in border)
    assert (nv[:, 2] == 0.0).all()
    assert abs(R.face_areas(nv, nf).sum() - 121.0) <= 1e-12 and (R.face_areas(nv, nf) > 0).all()
    assert R.euler(nv.shape[0], nf) == 1


def test_edge_of_three_faces_keeps_its_endpoints():
    v, f, (a, b) = R.finned_sphere()
    nv, nf, vmap = run(v, f, 100, return_map=True)
    assert nf.shape[0] in (100, 99)
    fixed = np.nonzero(vmap == np.arange(v.shape[0]))[0]
    for p in (a, b, v.shape[0] - 1):
        assert vmap[p] == p and np.array_equal(nv[np.searchsorted(fixed, p)], v[p])
    use = R.edge_use(nf)[1]
    assert (use == 3).sum() == 1 and (use == 1).sum() == 2


def test_hub_of_valence_40():
    v, f = R.hub(40)
    nv, nf = run(v, f, 40)
    assert nf.shape[0] == 40
    R.check_closed_manifold(nv, nf, 2)


def test_face_index_out_of_range_raises():
    v, f = R.icosphere(1)
    for bad in (v.shape[0], -1):
        g = f.copy()
        g[5, 1] = bad
        with pytest.raises(ValueError, match="outside"):
            run(v, g, 20)


@pytest.mark.parametrize("name", list(MESHES))
def test_quality_against_sequential_greedy(results, name):
    """Surface distance to the original, round scheme over sequential greedy (a heap, one collapse at a time, the same cost and
    validity rules - another schedule, not the code under test), at the same face count."""
    r = results[name]
    gv, gf = R.greedy_decimate(r["v"], r["f"], r["nf"].shape[0])
    assert gf.shape[0] == r["nf"].shape[0]
    ours, theirs = R.surface_distance(r["v"], r["f"], r["nv"], r["nf"]), R.surface_distance(r["v"], r["f"], gv, gf)
    ratio = ours / theirs
    print(f"{name}: round scheme {ours:.6e}, greedy {theirs:.6e}, ratio {ratio:.4f}")
    assert ratio <= MEASURED_RATIO[name] * 1.25, (ours, theirs, ratio)


def test_process_mesh_decimates_between_cleanup_and_floaters(monkeypatch):
    v, f = R.icosphere(2)
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    calls = []
    real_clean, real_decimate = MP._clean, MD.decimate_mesh
    monkeypatch.setattr(MP, "_clean", lambda *a, **k: (calls.append("clean"), real_clean(*a, **k))[1])
    monkeypatch.setattr(MD, "decimate_mesh", lambda *a, **k: (calls.append("decimate"), real_decimate(*a, backend=BACKEND, **k))[1])
    monkeypatch.setattr(MP.mesh_cleanup, "remove_floaters", lambda vv, ff, threshold: (calls.append(("floaters", ff.shape[0])), (vv, ff))[1])
    nv, nf = MP.process_mesh(tv, tf, face_decimation=100, floaters_threshold=0.01, decimation="hip")
    assert calls == ["clean", "decimate", ("floaters", 100)] and nf.shape[0] == 100
    want = real_decimate(tv, tf, 100, backend=BACKEND)
    assert torch.equal(nv, want[0]) and torch.equal(nf, want[1])
    calls.clear()
    MP.process_mesh(tv, tf, face_decimation=f.shape[0], floaters_threshold=0.0, decimation="hip")          # nothing to decimate
    assert calls == ["clean"]


def test_process_mesh_without_the_keyword_still_raises():
    v, f = R.icosphere(1)
    with pytest.raises(NotImplementedError, match="face_decimation"):
        MP.process_mesh(torch.from_numpy(v), torch.from_numpy(f), face_decimation=10)
    with pytest.raises(ValueError, match="decimation"):
        MP.process_mesh(torch.from_numpy(v), torch.from_numpy(f), face_decimation=10, decimation="cpu")
