"""Guard bands of the mesh kernels (am_mesh.hip): fp32 and int32 outputs in arenas of sentinels (tests/_guard.py), fp64 outputs in a
sentinel-padded buffer (Padded64), every input in a poisoned arena - NaN around the vertices, the prefix sum and the uniforms, an
index far outside the mesh around the faces and the CSR - so that a read past the last vertex, face, corner or sample shows up in the
values or in the entry point's flag.  Values against the restatements of tests/test_mesh_prep_gpu.py at its bounds."""
import numpy as np
import pytest
import torch

import test_mesh_prep_gpu as tg
from _guard import Arena, Padded64

pytestmark = pytest.mark.gpu

OUT_SENTINEL = -7.25e300


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from actionmesh_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _mesh(V, F, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(V, 3))
    f = np.stack([rng.choice(V, 3, replace=False) for _ in range(F)]).astype(np.int64)
    f[0, 0] = V - 1                                                              # the last vertex is read
    return v, f


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("F", [1, 129])
@pytest.mark.parametrize("V", [70, 64, 65])
def test_vertex_normals_guards(dev, V, F, dtype):
    """One workgroup covers 256 vertices or faces: V = 64 / 65 / 70 and F = 1 / 129 end inside a wave, at a wave's edge and one past
    it.  T = 2 frames with a padded frame stride."""
    from actionmesh_amd import mesh_prep as MP, ops
    T = 2
    v, f = _mesh(V, F, 100 * V + F)
    frames = np.stack((v, v * (1.5, 1.0, 0.5)))
    host = torch.from_numpy(frames).to(dtype)
    if dtype == torch.float32:
        VA = Arena(T, 3 * V, dtype, dev, ld=3 * V + 9)                           # frame stride 3 V + 9, NaN in the gaps and guards
        VA.view.copy_(host.reshape(T, 3 * V).to(dev))
        verts = torch.as_strided(VA.raw, (T, V, 3), (VA.ld, 3, 1), VA.origin)
    else:
        VP = Padded64((T, V + 3, 3), dev, float("nan"))
        VP.view[:, :V].copy_(host.to(dev))
        VP.before = VP.buf.clone()
        verts = VP.view[:, :V]
    topo = MP.MeshTopology(torch.from_numpy(f).to(dev), V)
    FA, OA, CA = (Arena.flat_of(t) for t in (topo.faces, topo.offsets, topo.corners))
    topo.faces, topo.offsets, topo.corners = FA.view, OA.view, CA.view
    out = Arena.flat((T, V, 6), torch.float32, dev)
    fn = Padded64((T, F, 3), dev, OUT_SENTINEL)
    got, got_fn = ops.vertex_normals(verts, FA.view, topology=topo, features=True, return_face_normals=True, out=out.view,
                                     out_face_normals=fn.view)
    torch.cuda.synchronize()
    assert got is out.view and got_fn is fn.view
    out.assert_untouched("features")
    fn.assert_untouched("face normals", written=True)
    for a, what in ((FA, "faces"), (OA, "offsets"), (CA, "corners")):
        a.assert_untouched(what)
    if dtype == torch.float32:
        VA.assert_untouched("vertices")
    else:
        VP.assert_untouched("vertices")
    widened = host.double().numpy()
    assert torch.equal(got[..., :3], host.float().to(dev))
    for t in range(T):
        want, want_fn = tg.ref_normals(widened[t], f)
        assert np.abs(got[t, :, 3:].cpu().numpy().astype(np.float64) - want).max() <= tg.NORMAL_TOL
        assert np.abs(got_fn[t].cpu().numpy() - want_fn).max() <= 1e-15
    plain = ops.vertex_normals(host.to(dev), torch.from_numpy(f).to(torch.int32).to(dev), features=True)
    assert torch.equal(plain.view(torch.int32), got.view(torch.int32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("F", [1, 129])
def test_face_areas_and_surface_sample_guards(dev, F, n, dtype):
    from actionmesh_amd import ops
    V = 65
    v, f = _mesh(V, F, 7 * F + n)
    host = torch.from_numpy(v).to(dtype)
    widened = host.double().numpy()
    if dtype == torch.float32:
        VA = Arena.flat_of(host.to(dev))
        verts = VA.view
    else:
        VA = Padded64((V, 3), dev, float("nan"), host.to(dev))
        verts = VA.view
    FA = Arena.flat_of(torch.from_numpy(f).to(torch.int32).to(dev))
    areas = Padded64((F,), dev, OUT_SENTINEL)
    assert ops.face_areas(verts, FA.view, out=areas.view) is areas.view
    torch.cuda.synchronize()
    areas.assert_untouched("areas", written=True)
    want_areas = tg.ref_faces(widened, f)[2] / 2.0
    assert (np.abs(areas.view.cpu().numpy() - want_areas) <= 2.3e-16 * want_areas).all()
    rng = np.random.default_rng(n)
    u_face, u_bary = rng.random(n), rng.random((n, 2))
    u_face[-1] = np.nextafter(1.0, 0.0)                                          # the last sample picks the last face
    cdf = Padded64((F,), dev, float("nan"), torch.cumsum(areas.view, 0))
    UF = Padded64((n,), dev, float("nan"), torch.from_numpy(u_face).to(dev))
    UB = Padded64((n, 2), dev, float("nan"), torch.from_numpy(u_bary).to(dev))
    points, normals = Padded64((n, 3), dev, OUT_SENTINEL), Padded64((n, 3), dev, OUT_SENTINEL)
    index = Arena.flat((n,), torch.int32, dev)
    got = ops.surface_sample(verts, FA.view, cdf.view, UF.view, UB.view, out_points=points.view, out_face_index=index.view,
                             out_normals=normals.view)
    torch.cuda.synchronize()
    assert got[0] is points.view and got[1] is index.view and got[2] is normals.view
    index.assert_untouched("face_index")
    points.assert_untouched("points", written=True)
    normals.assert_untouched("normals", written=True)
    for p, what in ((cdf, "cdf"), (UF, "u_face"), (UB, "u_bary")):
        p.assert_untouched(what)
    FA.assert_untouched("faces")
    VA.assert_untouched("vertices")
    want_face, want_points, want_normals = tg.ref_samples(widened, f, cdf.view.cpu().numpy(), u_face, u_bary)
    assert np.array_equal(index.view.cpu().numpy(), want_face) and want_face[-1] == F - 1
    assert np.array_equal(points.view.cpu().numpy().view(np.int64), want_points.view(np.int64))
    assert np.abs(normals.view.cpu().numpy() - want_normals).max() <= 1e-15
