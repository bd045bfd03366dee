"""The mesh kernels (csrc/am_mesh.hip) and the tensor interface over them (actionmesh_amd/mesh_prep.py) on the device, against numpy
fp64 restatements of the header's contract written out here step by step: every product, sum, division, sqrt and acos is one numpy
call, so it is rounded on its own as the kernel's is, and the vertex sums go through np.add.at over the corners in face-major order,
which is the CSR order."""
import numpy as np
import pytest
import torch

import test_mesh_prep_cpu as tm

pytestmark = pytest.mark.gpu

ZERO = 1e-13                    # AM_MESH_ZERO
NORMAL_TOL = 2.4e-7             # two fp32 ulps at 1.0: the fp64 part agrees with numpy to ~1e-15 (sqrt, acos, amplified by at most the
#                                 condition of acos at a 1 degree angle), far below fp32's 6e-8; what is left is the final rounding to
#                                 fp32 and the summation order of the fp32 re-normalisation


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from actionmesh_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---- the contract in numpy ----------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack((a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]), 1)


def ref_faces(v, f):
    """(unit face normals (F, 3), corner angles (F, 3), |c| (F,)) of fp64 vertices."""
    v0, v1, v2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    e1, e2, e3 = v1 - v0, v2 - v0, v2 - v1
    c = _cross(e1, e2)
    length = np.sqrt(_dot(c, c))
    ok = length > ZERO
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.where(ok[:, None], c / length[:, None], 0.0)
        u, w2, w = (e / np.sqrt(_dot(e, e))[:, None] for e in (e1, e2, e3))
        a0 = np.arccos(np.clip(_dot(u, w2), -1.0, 1.0))
        a1 = np.arccos(np.clip(-_dot(u, w), -1.0, 1.0))
        a2 = (np.pi - a0) - a1
    ang = np.where(ok[:, None], np.stack((a0, a1, a2), 1), 0.0)
    return n, ang, length


def ref_normals(v, f):
    """The fp32 vertex normals (V, 3) of one frame of fp64 vertices, and the unit face normals."""
    n, ang, _ = ref_faces(v, f)
    s = np.zeros((len(v), 3))
    np.add.at(s, f.reshape(-1), ang.reshape(-1, 1) * np.repeat(n, 3, axis=0))        # corner 3 * face + k, ascending
    length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = np.where((length > ZERO)[:, None], s / length[:, None], 0.0).astype(np.float32)
    l32 = np.sqrt((unit[:, 0] * unit[:, 0] + unit[:, 1] * unit[:, 1]) + unit[:, 2] * unit[:, 2])
    return unit / np.maximum(l32, np.float32(1e-12))[:, None], n


def ref_samples(v, f, cdf, u_face, u_bary):
    pick = u_face * cdf[-1]
    face = np.searchsorted(cdf, pick)
    r = u_bary.copy()
    fold = r[:, 0] + r[:, 1] > 1.0
    r[fold] = r[fold] - 1.0
    r = np.abs(r)
    v0, v1, v2 = v[f[face, 0]], v[f[face, 1]], v[f[face, 2]]
    points = (v0 + (v1 - v0) * r[:, :1]) + (v2 - v0) * r[:, 1:]
    return face, points, ref_faces(v, f)[0][face]


# ---- meshes: built once, never modified -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def meshes():
    a_v, a_f = tm.fan_mesh(zero_area_face=True)
    b_v, b_f = tm.icosphere(4)
    assert b_v.shape == (2562, 3) and b_f.shape == (5120, 3)
    _, ang, length = ref_faces(a_v, a_f)
    assert np.degrees(ang[length > ZERO].min()) >= 1.0 and int((length <= ZERO).sum()) == 1
    return {"a": (a_v, a_f), "b": (b_v, b_f)}


def _frames(v, T, dtype, dev):
    """(T, V, 3) frames of a mesh inside a buffer whose frame stride is above 3 V.  Frame t is the mesh scaled by (1 + t, 1, 2^-t):
    the normals differ from frame to frame, and the products are exact for the few-bit coordinates of the fan mesh's collinear face,
    which so stays a zero-area face in every frame and in fp32."""
    base = np.stack([v * (1.0 + t, 1.0, 2.0 ** -t) for t in range(T)])
    host = torch.from_numpy(base).to(dtype)
    if T == 1:
        return host.to(dev), host.double().numpy()
    buf = torch.full((T, v.shape[0] + 5, 3), float("nan"), dtype=dtype, device=dev)
    buf[:, :v.shape[0]] = host.to(dev)
    view = buf[:, :v.shape[0]]
    assert view.stride(0) > 3 * v.shape[0]
    return view, host.double().numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("name", ["a", "b"])
def test_vertex_normals_against_the_restatement(dev, meshes, name, T, dtype):
    from actionmesh_amd import mesh_prep as MP, ops
    v, f = meshes[name]
    verts, widened = _frames(v, T, dtype, dev)
    faces = torch.from_numpy(f).to(dev)
    topo = MP.MeshTopology(faces, len(v))
    feats, face_normals = ops.vertex_normals(verts, topo.faces, topology=topo, features=True, return_face_normals=True)
    assert feats.shape == (T, len(v), 6) and feats.dtype == torch.float32 and face_normals.shape == (T, len(f), 3)
    assert torch.equal(feats[..., :3], verts.float())                           # positions: the same bits
    worst = 0.0
    for t in range(T):
        want, want_faces = ref_normals(widened[t], f)
        if name == "a":
            _, ang, length = ref_faces(widened[t], f)
            assert np.degrees(ang[length > ZERO].min()) >= 1.0 and int((length <= ZERO).sum()) == 1
        got = feats[t, :, 3:].cpu().numpy()
        worst = max(worst, float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()))
        zero = ~want.any(axis=1)
        assert np.array_equal(got[zero], np.zeros_like(got[zero]))              # exactly 0.0, sign included below
        assert not np.signbit(got[zero]).any()
        assert np.abs(face_normals[t].cpu().numpy() - want_faces).max() <= 1e-15
        if name == "a":
            assert zero[68] and zero[69] and int(zero.sum()) == 2               # only a zero-area face touches 68; 69 is isolated
    print(f"mesh {name} T={T} {dtype}: worst |normal - restatement| {worst:.3e} (bound {NORMAL_TOL:.1e})")
    assert worst <= NORMAL_TOL
    again = ops.vertex_normals(verts, topo.faces, topology=topo, features=True)
    assert torch.equal(again.view(torch.int32), feats.view(torch.int32))        # two runs: the same bits
    normals = ops.vertex_normals(verts, topo.faces)                             # normals alone, topology built inside
    assert torch.equal(normals.view(torch.int32), feats[..., 3:].contiguous().view(torch.int32))
    got2 = MP.get_mesh_features(verts[0], faces, True)
    assert got2.shape == (len(v), 6) and torch.equal(got2.view(torch.int32), feats[0].view(torch.int32))
    assert torch.equal(MP.get_mesh_features(verts, faces, False), verts.float())


class _ZeroDisplacement:
    """Stands for the Stage-II decoder: no displacement, so every output timestep must hold the anchor's vertices."""

    def __init__(self, device):
        self.device = device
        self.queries = []

    def __call__(self, latent, framestep, source_alpha, target_alphas, query, step_callback=None):
        self.queries.append(query)
        return torch.zeros((1, target_alphas.shape[1], query.shape[1], 3), device=query.device)

    @staticmethod
    def apply_displacement(vertex, displacement, scale=1.0):
        return vertex[:, None] + displacement


def test_vertex_features_fits_generate_vertex_animation(dev, meshes):
    from actionmesh_amd import mesh_prep as MP, windows as W
    v, f = meshes["b"]
    verts, faces = torch.from_numpy(v).float().to(dev), torch.from_numpy(f).to(dev)
    features = MP.VertexFeatures(faces)
    assert features.topology is None
    got = features(verts)
    topo = features.topology
    assert torch.equal(got.view(torch.int32), MP.get_mesh_features(verts, faces, True).view(torch.int32))
    n_frames, N, D = 6, 4, 8
    ts = torch.arange(n_frames, dtype=torch.float32)
    bank = W.LatentBank(empty_dims=(N, D), device=str(dev))
    bank.update(ts, torch.zeros((n_frames, N, D), device=dev))
    vbank = W.LatentBank(empty_dims=(len(v), 3), device=str(dev))
    vbank.update(ts[:1], verts[None])
    ae = _ZeroDisplacement(dev)
    W.generate_vertex_animation(ae, bank, vbank, features, 0, 4, 3, device=dev)
    out, out_ts = vbank.get_ordered()
    assert out_ts.tolist() == ts.tolist() and len(ae.queries) == 2 and features.topology is topo
    assert all(torch.equal(q[0].view(torch.int32), got.view(torch.int32)) for q in ae.queries)
    assert all(torch.equal(frame, verts) for frame in out)


def _uniforms(n, seed):
    """Seeded uniforms with the edges planted: 0.0, the largest double below 1, and pairs whose sum is exactly 1."""
    rng = np.random.default_rng(seed)
    u_face, u_bary = rng.random(n), rng.random((n, 2))
    below_one = np.nextafter(1.0, 0.0)
    assert 1.0 - below_one <= 1.2e-16
    u_face[:4] = (0.0, below_one, 0.5, 0.0)
    u_bary[:6] = ((0.25, 0.75), (0.5, 0.5), (0.0, 0.0), (below_one, 0.0), (below_one, below_one), (0.0, below_one))
    assert u_bary[0].sum() == 1.0 and u_bary[1].sum() == 1.0
    return u_face, u_bary


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["20", "b"])
def test_surface_samples_against_the_restatement(dev, meshes, name, dtype):
    from actionmesh_amd import mesh_prep as MP, ops
    if name == "20":
        v, f = tm.icosphere(0)
        assert len(f) == 20
        dead = None
    else:
        v, f = meshes["b"]
        dead = len(f) // 2
        f = np.insert(f, dead, (f[7, 0], f[7, 0], f[7, 1]), axis=0)             # a zero-area face in the middle of the array
    n = 1000
    verts = torch.from_numpy(v).to(dtype).to(dev)
    widened = verts.double().cpu().numpy()
    faces = torch.from_numpy(f).to(torch.int32).to(dev)
    areas = ops.face_areas(verts, faces)
    want_areas = ref_faces(widened, f)[2] / 2.0
    assert (np.abs(areas.cpu().numpy() - want_areas) <= 2.3e-16 * want_areas).all()         # one ulp: sqrt, then an exact halving
    cdf = torch.cumsum(areas, 0)
    host_cdf = cdf.cpu().numpy()
    want_cdf = np.cumsum(want_areas)
    assert np.abs(host_cdf - want_cdf).max() <= len(f) * 2.3e-16 * want_cdf[-1]
    u_face, u_bary = _uniforms(n, 17)
    points, face_index, normals = ops.surface_sample(verts, faces, cdf, torch.from_numpy(u_face).to(dev), torch.from_numpy(u_bary).to(dev))
    want_face, want_points, want_normals = ref_samples(widened, f, host_cdf, u_face, u_bary)
    got_face = face_index.cpu().numpy()
    assert face_index.dtype == torch.int32 and np.array_equal(got_face, want_face)
    assert np.array_equal(points.cpu().numpy().view(np.int64), want_points.view(np.int64))       # bit-equal
    assert np.abs(normals.cpu().numpy() - want_normals).max() <= 1e-15
    assert got_face[0] == 0 and got_face[1] == len(f) - 1
    if dead is not None:
        assert want_areas[dead] == 0.0 and dead not in got_face
    # the tensor interface: the draws of sample_surface, the same kernel
    surface, idx2, cdf2 = MP.sample_surface(verts, torch.from_numpy(f).to(dev), n, seed=3, return_face_index=True)
    d_face, d_bary = MP.draw_uniforms(n, 3)
    w_face, w_points, w_normals = ref_samples(widened, f, cdf2.cpu().numpy(), d_face, d_bary)
    assert surface.shape == (1, n, 6) and surface.dtype == torch.float64 and torch.equal(cdf2, cdf)
    assert np.array_equal(idx2.cpu().numpy(), w_face) and np.array_equal(surface[0, :, :3].cpu().numpy(), w_points)
    assert np.abs(surface[0, :, 3:].cpu().numpy() - w_normals).max() <= 1e-15
    if dead is not None:
        assert dead not in idx2.cpu().numpy()
    half = MP.sample_surface(verts, torch.from_numpy(f).to(dev), n, seed=3, dtype=torch.float16)
    assert half.shape == (1, n, 6) and half.dtype == torch.float16 and half.device == verts.device
    assert torch.equal(half, surface.to(torch.float16))
    assert MP.sample_surface(verts, torch.from_numpy(f).to(dev), n, seed=3, with_normals=False, device="cpu").shape == (1, n, 3)


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g.cpu(), w), (g.shape, w.shape)


def test_merge_and_clean_on_the_device_equals_the_cpu_result(dev, meshes):
    from actionmesh_amd import mesh_prep as MP
    v, f, *_ = tm.hand_mesh()
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    _same(MP.merge_and_clean_mesh(tv.to(dev), tf.to(dev), return_index=True), MP.merge_and_clean_mesh(tv, tf, return_index=True))
    bv, bf = meshes["b"]
    dv, df = tm.dirty_copy(bv, bf, 300, 20, 20)
    assert len(dv) == len(bv) + 300 and len(df) == len(bf) + 40
    tv, tf = torch.from_numpy(dv), torch.from_numpy(df)
    got = MP.merge_and_clean_mesh(tv.to(dev), tf.to(dev), return_index=True)
    _same(got, MP.merge_and_clean_mesh(tv, tf, return_index=True))
    assert got[0].shape[0] == len(bv) and got[1].shape[0] == len(bf)
    _same(MP.process_mesh(tv.to(dev), tf.to(dev)), MP.process_mesh(tv, tf))
    # one component, so the floater removal behind the clean-up returns its input
    _same(MP.process_mesh(tv.to(dev), tf.to(dev), floaters_threshold=0.5), MP.process_mesh(tv, tf))


def test_the_chain_returns_the_original_topology(dev, meshes):
    """merge_and_clean_mesh -> normalize_mesh -> (features, samples) -> denormalize_mesh -> expand_to_original: the original vertex
    array to 1e-6, and pre_merge_faces unchanged."""
    from actionmesh_amd import mesh_prep as MP
    bv, bf = meshes["b"]
    dv, df = tm.dirty_copy(bv * 3.0 + (5.0, -2.0, 1.0), bf, 300, 20, 20)
    tv, tf = torch.from_numpy(dv).to(dev), torch.from_numpy(df).to(dev)
    keep = tf.clone()
    cv, cf, merge_map, pre = MP.merge_and_clean_mesh(tv, tf)
    nv, params = MP.normalize_mesh(cv)
    assert float(nv.abs().max()) <= 1.0 + 1e-12
    feats = MP.get_mesh_features(nv, cf, True)
    surface = MP.sample_surface(nv, cf, 256, seed=0)
    assert feats.shape == (cv.shape[0], 6) and surface.shape == (1, 256, 6) and bool(torch.isfinite(feats).all())
    frames = torch.stack((nv, nv))                                              # what Stage II hands back: (T, V, 3)
    out = MP.expand_to_original(MP.denormalize_mesh(frames, params), merge_map)
    assert out.shape == (2, len(dv), 3) and float((out - tv).abs().max()) <= 1e-6
    assert pre is tf and torch.equal(tf, keep)


@pytest.mark.parametrize("bad", ["V", "-1"])
def test_an_out_of_range_face_index_is_an_error_return(dev, bad):
    """The kernels compare every index with its bound before using it: the call returns, the flag is set, the wrapper raises."""
    from actionmesh_amd import ops
    v, f = tm.fan_mesh()
    g = f.copy()
    g[37, 1] = len(v) if bad == "V" else -1
    verts, faces = torch.from_numpy(v).to(dev), torch.from_numpy(g).to(torch.int32).to(dev)
    with pytest.raises(ValueError, match=r"vertex_normals: a face names a vertex outside \[0, 70\)"):
        ops.vertex_normals(verts, faces)
    with pytest.raises(ValueError, match=r"face_areas: a face names a vertex outside \[0, 70\)"):
        ops.face_areas(verts, faces)
    cdf = torch.arange(1, len(g) + 1, dtype=torch.float64, device=dev)
    u = torch.full((4,), 37.5 / len(g), dtype=torch.float64, device=dev)          # picks face 37
    with pytest.raises(ValueError, match=r"surface_sample: a face names a vertex outside \[0, 70\)"):
        ops.surface_sample(verts, faces, cdf, u, torch.zeros((4, 2), dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    good = torch.from_numpy(f).to(torch.int32).to(dev)
    assert bool(torch.isfinite(ops.vertex_normals(verts, good)).all())           # and the device goes on working
