"""Host logic of actionmesh_amd/mesh_prep.py that needs no kernel, on CPU tensors: the vertex -> corner CSR, the normalisation
formulas of the reference restated in numpy, the order of sample_surface's random draws, process_mesh's refusal of decimation, and
the four clean-up steps of merge_and_clean_mesh on a mesh small enough to write the answer by hand.  The mesh builders here are shared
with tests/test_mesh_prep_gpu.py and tests/test_guard_mesh_gpu.py."""
import numpy as np
import pytest
import torch

from actionmesh_amd import mesh_prep as MP


# ---- meshes -----------------------------------------------------------------------------------------------------------------------------
def fan_mesh(zero_area_face: bool = False):
    """V = 70: vertex 0 is the centre of a fan of 40 triangles over the ring 1..40 (valence 40), 41..67 are a strip of 25 triangles,
    68 lies midway between 41 and 43 and 69 is far away; neither is referenced by a face.  With `zero_area_face` the collinear face
    (41, 68, 43) is added in the middle of the face array, so vertex 68 is touched by a zero-area face only.  fp64 (V, 3), int64 (F, 3)."""
    v = np.zeros((70, 3))
    v[0] = (0.0, 0.0, 0.3)
    ang = 2 * np.pi * np.arange(40) / 40
    v[1:41] = np.stack((np.cos(ang), np.sin(ang), 0.05 * np.cos(3 * ang)), 1)
    i = np.arange(27)
    v[41:68] = np.stack((3.0 + 0.5 * i, 0.8 * (i % 2), 0.125 * i), 1)
    v[68] = (v[41] + v[43]) / 2
    v[69] = (-4.0, 5.0, 6.0)
    fan = [(0, 1 + k, 1 + (k + 1) % 40) for k in range(40)]
    strip = [(41 + k, 42 + k, 43 + k) if k % 2 == 0 else (42 + k, 41 + k, 43 + k) for k in range(25)]
    faces = fan[:20] + strip + fan[20:]
    if zero_area_face:
        faces = faces[:33] + [(41, 68, 43)] + faces[33:]
    return v, np.asarray(faces, dtype=np.int64)


def icosphere(subdivisions: int = 4, jitter: float = 1e-2, seed: int = 5):
    """An icosahedron subdivided `subdivisions` times onto the unit sphere (4: V = 2562, F = 5120), every coordinate moved by a seeded
    uniform in (-jitter, jitter).  fp64 (V, 3), int64 (F, 3)."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
             (-t, 0, -1), (-t, 0, 1)]
    verts = [np.asarray(p, dtype=np.float64) / np.linalg.norm(p) for p in verts]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]
        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    v = np.asarray(verts)
    v = v + np.random.default_rng(seed).uniform(-jitter, jitter, v.shape)
    return v, np.asarray(faces, dtype=np.int64)


def hand_mesh(isolated_vertex: bool = False):
    """The 12-vertex mesh of the clean-up test, and what merge_and_clean_mesh must make of it.
      vertex 7 is vertex 1 moved by 4e-9 (a seam duplicate: merges), vertex 8 is vertex 2 moved by 2e-8 (must NOT merge), vertex 10
      is a copy of vertex 0 that no face references (merges into 0); face 4 repeats an index, face 12 does so after the merge, face 5
      is collinear, face 8 is face 0 with reversed winding.
    With `isolated_vertex` a 13th vertex far from everything is appended: it is unreferenced and has no image in the cleaned mesh.
    Returns (vertices fp64, faces int64, expected vertices', faces', vertex_merge_map, kept face indices)."""
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [2, 0, 0], [2, 1, 0], [0.5, 0.5, 1], [1 + 4e-9, 0, 0], [1, 1 + 2e-8, 0],
                  [1.5, 0, 0], [0, 0, 0], [3, 0.5, 0]], dtype=np.float64)
    f = np.array([[0, 1, 2], [0, 2, 3], [7, 4, 5], [7, 5, 2], [0, 0, 3], [1, 9, 4], [1, 9, 6], [9, 4, 6], [2, 1, 0], [8, 5, 6],
                  [4, 11, 5], [0, 6, 3], [1, 7, 4]], dtype=np.int64)
    new_v = v[[0, 1, 2, 3, 4, 5, 6, 8, 9, 11]]
    new_f = np.array([[0, 1, 2], [0, 2, 3], [1, 4, 5], [1, 5, 2], [1, 8, 6], [8, 4, 6], [7, 5, 6], [4, 9, 5], [0, 6, 3]], dtype=np.int64)
    merge_map = np.array([0, 1, 2, 3, 4, 5, 6, 1, 7, 8, 0, 9], dtype=np.int64)
    kept = np.array([0, 1, 2, 3, 6, 7, 9, 10, 11], dtype=np.int64)
    if isolated_vertex:
        v = np.concatenate((v, [[9.0, 9.0, 9.0]]))
        merge_map = np.concatenate((merge_map, [-1]))
    return v, f, new_v, new_f, merge_map, kept


def dirty_copy(v, f, n_seam: int, n_degenerate: int, n_duplicate: int, seed: int = 11):
    """A clean mesh made dirty the way a GLB loader does it: `n_seam` seeded vertices are duplicated (moved by up to 3e-9) and a
    seeded half of the corners that named the original now name the copy; `n_degenerate` faces with a repeated index and
    `n_duplicate` copies of existing faces (every second with reversed winding) are inserted at seeded positions."""
    rng = np.random.default_rng(seed)
    v, f = v.copy(), f.copy()
    seam = rng.choice(len(v), n_seam, replace=False)
    copies = v[seam] + rng.uniform(-3e-9, 3e-9, (n_seam, 3))
    # keep the copy on the same side of a rounding boundary of the 1e-8 grid as the original: the merge is by rounded key
    copies = np.where(np.round(copies * 1e8) == np.round(v[seam] * 1e8), copies, v[seam])
    new_id = {int(s): len(v) + k for k, s in enumerate(seam)}
    v = np.concatenate((v, copies))
    flat = f.reshape(-1)
    for c in np.nonzero(np.isin(flat, seam) & (rng.random(flat.size) < 0.5))[0]:
        flat[c] = new_id[int(flat[c])]
    f = flat.reshape(-1, 3)
    extra = []
    for k in range(n_degenerate):
        a, b = rng.choice(len(v), 2, replace=False)
        extra.append((a, b, a))
    for k in range(n_duplicate):
        a, b, c = f[rng.integers(len(f))]
        extra.append((c, b, a) if k % 2 else (b, c, a))
    for face in extra:
        f = np.insert(f, rng.integers(len(f) + 1), face, axis=0)
    return v, f


# ---- tests ------------------------------------------------------------------------------------------------------------------------------
def test_topology_csr_against_a_dictionary():
    """For every vertex the corner list equals a brute-force dictionary's, in ascending corner id; the fan centre has valence 40 and
    the unreferenced vertices have empty lists."""
    v, f = fan_mesh()
    topo = MP.MeshTopology(torch.from_numpy(f), len(v))
    assert topo.offsets.dtype == torch.int32 and topo.corners.dtype == torch.int32 and topo.faces.dtype == torch.int32
    assert topo.offsets.shape == (71,) and topo.corners.shape == (3 * len(f),)
    want = {i: [] for i in range(len(v))}
    for face in range(len(f)):
        for k in range(3):
            want[int(f[face, k])].append(3 * face + k)
    off, cor = topo.offsets.tolist(), topo.corners.tolist()
    assert off[0] == 0 and off[-1] == 3 * len(f)
    for i in range(len(v)):
        got = cor[off[i]:off[i + 1]]
        assert got == want[i] and got == sorted(got), i
    assert off[1] - off[0] == 40 and off[69] == off[70] and off[68] == off[69]


def test_topology_leaves_out_of_range_indices_to_the_kernel():
    """An index outside [0, V) lands in no vertex's list (the kernel reports it through its flag): building raises nothing and reads
    nothing back."""
    f = torch.tensor([[0, 1, 2], [2, 3, -1], [3, 4, 1]])
    topo = MP.MeshTopology(f, 4)
    off, cor = topo.offsets.tolist(), topo.corners.tolist()
    assert [cor[off[i]:off[i + 1]] for i in range(4)] == [[0], [1, 8], [2, 3], [4, 6]]


def _normalize_numpy(v, center):
    """The reference's normalize_mesh (mesh_processor.py:177-212) on an array."""
    v = v.copy()
    bbox_center = None
    if center:
        bbox_center = (v.min(axis=0) + v.max(axis=0)) / 2.0
        v -= bbox_center
    scale = (v.max(axis=0) - v.min(axis=0)).max()
    if scale > 0:
        v *= 2.0 / scale
    return v, bbox_center, scale


@pytest.mark.parametrize("center", [True, False])
def test_normalize_and_denormalize_follow_the_reference_formulas(center):
    v = np.random.default_rng(3).normal(size=(200, 3)) * (3.0, 0.7, 1.9) + (10.0, -2.0, 0.5)
    got, params = MP.normalize_mesh(torch.from_numpy(v), center=center)
    want, bbox_center, scale = _normalize_numpy(v, center)
    assert np.array_equal(got.numpy(), want)                                # exactly, in fp64
    assert float(params.scale) == scale
    assert (params.bbox_center is None) if not center else np.array_equal(params.bbox_center.numpy(), bbox_center)
    back = want * (scale / 2.0)
    if center:
        back = back + bbox_center
    assert np.array_equal(MP.denormalize_mesh(got, params).numpy(), back)
    assert np.abs(back - v).max() < 1e-13 and float(got.amax(0).sub(got.amin(0)).max()) <= 2.0 + 1e-15
    if center:
        assert float(got.abs().max()) <= 1.0 + 1e-15
    frames = torch.stack((got, got * 0.5, got + 0.1))                       # (T, V, 3)
    assert np.array_equal(MP.denormalize_mesh(frames, params)[1].numpy(), MP.denormalize_mesh(got * 0.5, params).numpy())
    v32 = torch.from_numpy(v).float()
    got32, params32 = MP.normalize_mesh(v32)
    assert got32.dtype == torch.float32 and params32.scale.dtype == torch.float32


def test_normalize_leaves_a_mesh_without_extent_unscaled():
    p = torch.tensor([[1.5, -2.0, 3.0]], dtype=torch.float64)
    got, params = MP.normalize_mesh(p)
    assert float(params.scale) == 0.0 and torch.equal(got, torch.zeros_like(p))
    assert torch.equal(MP.denormalize_mesh(got, params), p)
    got, params = MP.normalize_mesh(p, center=False)
    assert float(params.scale) == 0.0 and params.bbox_center is None and torch.equal(got, p)
    assert torch.equal(MP.denormalize_mesh(got, params), p)


def test_normalize_to_bounds():
    """Inside the bounds: the same bits.  Outside: the reference's formula (mesh_processor.py:348-365) restated in numpy."""
    v = np.random.default_rng(4).normal(size=(50, 3))
    small = torch.from_numpy(v / np.abs(v).max() * 0.9)
    assert torch.equal(MP.normalize_mesh_to_bounds(small), small)
    big = v * 3.0 + 0.5
    bounds = (-1.005,) * 3 + (1.005,) * 3
    tmin, tmax = np.array(bounds[:3]), np.array(bounds[3:])
    mmin, mmax = big.min(0), big.max(0)
    scale = min(1.0, ((tmax - tmin) / np.maximum(mmax - mmin, 1e-8)).min())
    want = (big - (mmin + mmax) / 2) * scale + (tmin + tmax) / 2
    assert np.array_equal(MP.normalize_mesh_to_bounds(torch.from_numpy(big), bounds).numpy(), want)


@pytest.mark.parametrize("seed", [0, 7])
def test_sample_surface_draws_its_uniforms_in_trimesh_order(monkeypatch, seed):
    """The uniforms that reach the kernel are default_rng(seed).random(n), then .random((n, 2, 1)) - trimesh's calls, in its order."""
    seen = {}

    def fake_areas(vertices, faces):
        return torch.ones(faces.shape[0], dtype=torch.float64)

    def fake_sample(vertices, faces, cdf, u_face, u_bary, with_normals=True):
        seen.update(cdf=cdf.clone(), u_face=u_face.clone(), u_bary=u_bary.clone())
        n = u_face.numel()
        return torch.zeros((n, 3), dtype=torch.float64), torch.zeros(n, dtype=torch.int32), torch.ones((n, 3), dtype=torch.float64)
    monkeypatch.setattr(MP.ops, "face_areas", fake_areas)
    monkeypatch.setattr(MP.ops, "surface_sample", fake_sample)
    v, f = fan_mesh()
    n = 37
    out = MP.sample_surface(torch.from_numpy(v), torch.from_numpy(f), n, seed=seed, dtype=torch.float16)
    assert out.shape == (1, n, 6) and out.dtype == torch.float16
    random = np.random.default_rng(seed).random
    assert np.array_equal(seen["u_face"].numpy(), random(n))
    assert np.array_equal(seen["u_bary"].numpy(), random((n, 2, 1)).reshape(n, 2))
    assert np.array_equal(seen["cdf"].numpy(), np.arange(1, len(f) + 1, dtype=np.float64))
    surface, face_index, cdf = MP.sample_surface(torch.from_numpy(v), torch.from_numpy(f), n, seed=seed, with_normals=False,
                                                 return_face_index=True)
    assert surface.shape == (1, n, 3) and surface.dtype == torch.float64 and face_index.shape == (n,) and cdf.shape == (len(f),)


def test_sample_surface_without_a_seed_uses_the_global_generator(monkeypatch):
    state = np.random.get_state()
    try:
        np.random.seed(123)
        u_face, u_bary = MP.draw_uniforms(5, seed=None)
        np.random.seed(123)
        assert np.array_equal(u_face, np.random.random(5)) and np.array_equal(u_bary, np.random.random((5, 2, 1)).reshape(5, 2))
    finally:
        np.random.set_state(state)


def test_process_mesh_refuses_decimation_by_name():
    v, f, new_v, new_f, _, _ = hand_mesh()
    with pytest.raises(NotImplementedError, match="face_decimation"):
        MP.process_mesh(torch.from_numpy(v), torch.from_numpy(f), face_decimation=5)
    got_v, got_f = MP.process_mesh(torch.from_numpy(v), torch.from_numpy(f), face_decimation=len(new_f))      # at the target: skipped
    assert np.array_equal(got_v.numpy(), new_v) and np.array_equal(got_f.numpy(), new_f)


def test_merge_and_clean_on_the_hand_built_mesh():
    """Expected arrays written out by hand (hand_mesh)."""
    v, f, new_v, new_f, merge_map, kept = hand_mesh()
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    got_v, got_f, got_map, pre, got_kept = MP.merge_and_clean_mesh(tv, tf, return_index=True)
    assert pre is tf and got_v.dtype == tv.dtype and got_f.dtype == tf.dtype and got_map.dtype == torch.int64
    assert np.array_equal(got_v.numpy(), new_v) and np.array_equal(got_f.numpy(), new_f)
    assert np.array_equal(got_map.numpy(), merge_map) and np.array_equal(got_kept.numpy(), kept)
    assert np.abs(got_v.numpy()[got_map.numpy()] - v).max() <= 1e-8
    assert len(MP.merge_and_clean_mesh(tv, tf)) == 4
    assert torch.equal(MP.expand_to_original(got_v, got_map), got_v[got_map])
    frames = torch.stack((got_v, got_v + 1))
    assert torch.equal(MP.expand_to_original(frames, got_map)[1], got_v[got_map] + 1)
    # fp32 vertices and int32 faces keep their dtypes (at 1.0 the 4e-9 and 2e-8 offsets are below a float's spacing: 7 and 8 both merge)
    v32, f32, map32, _ = MP.merge_and_clean_mesh(tv.float(), tf.int())
    assert v32.dtype == torch.float32 and f32.dtype == torch.int32 and v32.shape[0] == 9 and torch.equal(v32[map32], tv.float())


def test_an_original_vertex_without_an_image_is_an_assertion_error():
    """A vertex no face references and nothing merges with has no image in the cleaned mesh: the reference's distance assertion fails
    there, and so does this one, with its message.  process_mesh, which returns no map, drops the vertex and keeps the order of the rest."""
    v, f, new_v, new_f, _, _ = hand_mesh(isolated_vertex=True)
    with pytest.raises(AssertionError, match="Some pre-merge vertices have no close match in the merged mesh"):
        MP.merge_and_clean_mesh(torch.from_numpy(v), torch.from_numpy(f))
    got_v, got_f = MP.process_mesh(torch.from_numpy(v), torch.from_numpy(f))
    assert np.array_equal(got_v.numpy(), new_v) and np.array_equal(got_f.numpy(), new_f)


def test_clean_up_refuses_a_face_index_outside_the_vertices():
    v, f, *_ = hand_mesh()
    for bad in (len(v), -1):
        g = f.copy()
        g[3, 1] = bad
        with pytest.raises(ValueError, match="outside"):
            MP.merge_and_clean_mesh(torch.from_numpy(v), torch.from_numpy(g))


def test_dirty_copy_cleans_back_to_the_clean_mesh():
    """The seeded dirty mesh of the device test: cleaning returns the clean topology's face count and every original position."""
    v, f = icosphere(2)
    dv, df = dirty_copy(v, f, 30, 5, 5)
    got_v, got_f, got_map, pre = MP.merge_and_clean_mesh(torch.from_numpy(dv), torch.from_numpy(df))
    assert got_v.shape[0] == len(v) and got_f.shape[0] == len(f) and pre.shape[0] == len(f) + 10
    assert float((got_v[got_map] - torch.from_numpy(dv)).abs().max()) <= 1e-8
