"""Iso-surface extraction without a device: the shipped Python (actionmesh_amd/isosurface.py) on CPU tensors, with the numpy
restatement of the header's contract (tests/_isosurface_ref.py) in place of the kernels.

* invariants of the extracted surfaces: vertex / face counts and Euler characteristic, every edge in two faces, every directed edge
  once, every vertex used, orientation, enclosed volume - the figures are those of the contract, measured on a prototype that
  follows the same rules, not of the code under test;
* open surfaces, non-finite samples, empty results, the smallest and a non-cubic grid;
* the hierarchy against the dense extraction, bit for bit;
* the chain into `merge_and_clean_mesh` and `decimate_mesh`;
* the seam: the reference's own `TripoSGVAE.decode_latents` reaches the installed function.
"""
import importlib
import inspect
import logging
import os
import sys
import types

import numpy as np
import pytest
import torch

import _isosurface_ref as R
from actionmesh_amd import cli, dropin
from actionmesh_amd import isosurface as ISO

REF = "/root/reference"
HAVE_REF = os.path.isdir(os.path.join(REF, "actionmesh"))
BACKEND = R.NumpyBackend()
_cache = {}


def extract(name, n=None):
    """The shipped wrapper on one of the fields, once per case: (vertices, faces) as numpy arrays."""
    if (name, n) not in _cache:
        if name == "octahedron":
            values, frame = R.octahedron(), {}
        else:
            values = {"sphere": R.sphere, "torus": R.torus, "two_spheres": R.two_spheres}[name](n)
            frame = dict(zip(("origin", "spacing"), R.frame(n)))
        v, f = ISO.extract_isosurface(torch.from_numpy(values), backend=BACKEND, **frame)
        assert v.dtype == torch.float32 and f.dtype == torch.int64 and v.shape[1:] == (3,) and f.shape[1:] == (3,)
        _cache[(name, n)] = (v.numpy(), f.numpy())
    return _cache[(name, n)]


# ---- invariants --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, n, V, F, chi", [("sphere", 9, 590, 1176, 2), ("sphere", 17, 2318, 4632, 2), ("sphere", 33, 9248, 18492, 2),
                                                 ("torus", 17, 1552, 3104, 0), ("torus", 33, 6556, 13112, 0),
                                                 ("two_spheres", 17, 652, 1296, 4), ("octahedron", None, 194, 384, 2)])
def test_counts_and_closed_oriented_manifold(name, n, V, F, chi):
    v, f = extract(name, n)
    assert (v.shape[0], f.shape[0]) == (V, F)
    R.check_closed_oriented(v, f, chi)
    assert R.signed_volume(v, f) > 0


def test_octahedron_volume():
    """Integer samples on integer coordinates, many of them equal to the level: the surface is the octahedron |i - 4| + |j - 4| +
    |k - 4| = 3 of volume 36.  The contract's positions are exact to a few fp64 roundings (t is 0, 1/2, 1/3 or 2/3) and are then
    rounded once to fp32, so the bound of 1e-9 is held on the fp64 positions, the shipped fp32 ones must be exactly their rounding,
    and their volume is held to what that rounding allows: surface area 8 * (sqrt(3) / 4) * 18 = 62.4 times the largest
    displacement sqrt(3) * 2^-22 (half an ulp below 8 per component) = 2.6e-5 (measured: 1.8e-7)."""
    values = R.octahedron()
    mask, count = R.ref_classify(values)
    voff, toff, V, F = R.offsets_of(mask, count)
    v, f = extract("octahedron")
    idx_faces = R.ref_triangles(values, mask, count, voff, toff, V, F).astype(np.int64)
    assert np.array_equal(idx_faces, f) and V == v.shape[0]
    exact = _fp64_positions(values, mask)
    assert abs(R.signed_volume(exact, f) - 36.0) <= 1e-9
    assert np.array_equal(exact.astype(np.float32), v)
    print("octahedron: fp32 volume - 36 =", R.signed_volume(v, f) - 36.0)
    assert abs(R.signed_volume(v, f) - 36.0) <= 62.4 * 3 ** 0.5 * 2.0 ** -22


def _fp64_positions(values, mask):
    """The contract's vertex positions before the rounding to fp32, index frame, level 0."""
    flat = mask.reshape(-1)
    points = np.nonzero(flat)[0]
    row, col = np.nonzero((flat[points, None] >> np.arange(7)) & 1)
    p, m = points[row], col + 1
    a = np.stack(np.unravel_index(p, values.shape), axis=1)
    b = a + np.stack((m >> 2 & 1, m >> 1 & 1, m & 1), axis=1)
    va, vb = values.astype(np.float64)[tuple(a.T)], values.astype(np.float64)[tuple(b.T)]
    t = (0.0 - va) / (vb - va)
    return a + t[:, None] * (b - a).astype(np.float64)


def test_volume_converges_to_the_analytic_one():
    sphere = [R.signed_volume(*extract("sphere", n)) / R.SPHERE_VOLUME for n in (9, 17, 33)]
    torus = [R.signed_volume(*extract("torus", n)) / R.TORUS_VOLUME for n in (17, 33)]
    print("volume / analytic: sphere", sphere, "torus", torus)
    assert abs(sphere[2] - 1) < 0.01 and abs(torus[1] - 1) < 0.02
    assert sphere[0] < sphere[1] < sphere[2] and torus[0] < torus[1]


def test_normals_point_down_the_gradient():
    """Every non-degenerate face (fp64 area >= 1e-12) of the 17^3 sphere: normal . (-grad field) > 0 at the centroid; no face of the
    sphere is degenerate.  The octahedron's exact hits give degenerate faces: their number is reported, the others are held to the
    same with the outward direction of the convex body."""
    v, f = extract("sphere", 17)
    normal, area = R.face_normals_and_areas(v, f)
    assert (area >= 1e-12).all()
    centroid = v.astype(np.float64)[f].mean(axis=1)
    outward = centroid - np.asarray(R.SPHERE_CENTRE)               # -grad(r - |x - c|) = (x - c) / |x - c|
    assert (np.einsum("ij,ij->i", normal, outward) > 0).all()
    v, f = extract("octahedron")
    normal, area = R.face_normals_and_areas(v, f)
    keep = area >= 1e-12
    print("octahedron: degenerate faces", int((~keep).sum()), "of", f.shape[0])
    centroid = v.astype(np.float64)[f].mean(axis=1) - 4.0
    assert (np.einsum("ij,ij->i", normal, np.sign(centroid))[keep] > 0).all()      # -grad of 3 - |x - 4|_1 is sign(x - 4)


def test_inside_below_on_the_negated_field_is_the_identical_mesh():
    v, f = extract("sphere", 17)
    o, s = R.frame(17)
    nv, nf = ISO.extract_isosurface(torch.from_numpy(-R.sphere(17)), origin=o, spacing=s, inside="below", backend=BACKEND)
    assert np.array_equal(nv.numpy().view(np.uint32), v.view(np.uint32)) and np.array_equal(nf.numpy(), f)
    # and the other side of the same values is the same surface with the reverse winding
    rv, rf = ISO.extract_isosurface(torch.from_numpy(R.sphere(17)), origin=o, spacing=s, inside="below", backend=BACKEND)
    assert rv.shape == v.shape and rf.shape == f.shape and R.signed_volume(rv.numpy(), rf.numpy()) < 0


def test_random_field_is_an_open_manifold_with_and_without_nans():
    r = np.random.default_rng(0).standard_normal((7, 7, 7)).astype(np.float32)
    for with_nans in (False, True):
        if with_nans:
            r[2, 3, 4] = r[5, 5, 1] = np.nan
        v, f = ISO.extract_isosurface(torch.from_numpy(r), backend=BACKEND)
        uses = R.edge_use_counts(f.numpy())
        assert (uses <= 2).all() and (uses == 1).any()
        assert R.directed_edges_unique(f.numpy()) and R.all_vertices_used(v.shape[0], f.numpy())
    # the restatement without the wrapper's compaction has vertices that no face uses: only next to the non-finite samples
    rv, rf = R.ref_extract(r, compact=False)
    assert np.unique(rf).shape[0] == v.shape[0] < rv.shape[0]
    assert np.array_equal(rv[np.unique(rf)], v.numpy())


def test_surface_cut_by_the_grid_border_is_open():
    x, y, z = R.axes(9)
    v, f = ISO.extract_isosurface(torch.from_numpy(R.sphere_of(x, y, z, 1.2, (0, 0, 0)).astype(np.float32)), bounds=(-1,) * 3 + (1,) * 3,
                                  backend=BACKEND)
    uses = R.edge_use_counts(f.numpy())
    assert f.shape[0] > 0 and (uses == 1).any() and (uses <= 2).all()
    assert ISO.border_edge_count(f) == int((uses == 1).sum())
    assert float(v.abs().max()) <= 1.0


@pytest.mark.parametrize("fill", [1.0, -1.0, float("nan")])
def test_grids_without_a_crossing_are_empty(fill):
    v, f = ISO.extract_isosurface(torch.full((5, 6, 7), fill), backend=BACKEND)
    assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == torch.float32 and f.dtype == torch.int64


def test_smallest_grid():
    values = torch.full((2, 2, 2), -1.0)
    values[0, 0, 0] = 1.0
    v, f = ISO.extract_isosurface(values, backend=BACKEND)
    assert v.shape == (7, 3) and f.shape == (6, 3)                 # the corner all six tetrahedra share: one triangle each
    assert np.array_equal(v.numpy()[[0, 1, 3]], 0.5 * np.eye(3, dtype=np.float32)[::-1])     # edges 001, 010, 100 at their midpoints


def test_noncubic_anisotropic_equals_the_restatement():
    values, origin, spacing = R.noncubic_with_nans()
    v, f = ISO.extract_isosurface(torch.from_numpy(values), origin=origin, spacing=spacing, backend=BACKEND)
    rv, rf = R.ref_extract(values, 0.0, origin, spacing)
    assert f.shape[0] > 500 and np.array_equal(v.numpy().view(np.uint32), rv.view(np.uint32)) and np.array_equal(f.numpy(), rf)
    # a level other than 0, and bounds instead of origin / spacing
    hi = tuple(o + s * (n - 1) for o, s, n in zip(origin, spacing, values.shape))
    v, f = ISO.extract_isosurface(torch.from_numpy(values), level=0.25, bounds=origin + hi, backend=BACKEND)
    sp = tuple((h - o) / (n - 1) for o, h, n in zip(origin, hi, values.shape))
    rv, rf = R.ref_extract(values, 0.25, origin, sp)
    assert np.array_equal(v.numpy().view(np.uint32), rv.view(np.uint32)) and np.array_equal(f.numpy(), rf)


def test_argument_validation():
    ok = torch.zeros((3, 3, 3))
    for bad, exc in ((torch.zeros((3, 3)), ValueError), (torch.zeros((1, 3, 3)), ValueError), (ok.double(), TypeError)):
        with pytest.raises(exc):
            ISO.extract_isosurface(bad, backend=BACKEND)
    with pytest.raises(ValueError, match="inside"):
        ISO.extract_isosurface(ok, inside="left", backend=BACKEND)
    with pytest.raises(ValueError, match="finite"):
        ISO.extract_isosurface(ok, level=float("nan"), backend=BACKEND)
    with pytest.raises(ValueError, match="not both"):
        ISO.extract_isosurface(ok, bounds=1.0, origin=(0, 0, 0), backend=BACKEND)
    with pytest.raises(RuntimeError):                              # no CPU path: the shipped backend refuses a CPU tensor
        ISO.extract_isosurface(ok)


def test_the_restatement_derives_the_table_it_uses():
    """Fourteen cases per tetrahedron, one triangle for 1 or 3 inside corners and two for 2; mirrored tetrahedra (odd permutations)
    carry the reversed polygons; complementary masks carry the opposite windings."""
    pop = np.array([bin(c).count("1") for c in range(16)])
    assert np.array_equal(R.TRI_COUNT, np.tile(np.array([0, 1, 2, 1, 0])[pop], (6, 1)))
    assert R.CORNER.tolist() == [[0, 4, 6, 7], [0, 4, 5, 7], [0, 2, 6, 7], [0, 2, 3, 7], [0, 1, 5, 7], [0, 1, 3, 7]]
    for t in range(6):
        for case in range(1, 15):
            tris = R.TRI_EDGE[t, case, :R.TRI_COUNT[t, case]]
            assert (tris[..., 0] < tris[..., 1]).all()
            assert all(((case >> a) & 1) != ((case >> b) & 1) for a, b in tris.reshape(-1, 2))      # every vertex on a crossing edge
    assert np.array_equal(R.TRI_EDGE[0], R.TRI_EDGE[3]) and not np.array_equal(R.TRI_EDGE[0], R.TRI_EDGE[1])


# ---- hierarchy -----------------------------------------------------------------------------------------------------------------------
BOUNDS = (-1.005,) * 3 + (1.005,) * 3


def _field_f32(kind, x, y, z):
    """The field in float32 arithmetic on float32 coordinates (numpy arrays)."""
    if kind == "sphere":
        return (0.8 - np.sqrt((x - 0.03) ** 2 + (y + 0.02) ** 2 + (z - 0.01) ** 2)).astype(np.float32)
    return (0.25 - np.sqrt((np.sqrt(x ** 2 + y ** 2) - 0.6) ** 2 + z ** 2)).astype(np.float32)


def _dense(kind, n):
    if ("dense", kind, n) not in _cache:
        x = np.linspace(-1.005, 1.005, n).astype(np.float32)
        values = _field_f32(kind, *np.meshgrid(x, x, x, indexing="ij"))
        v, f = ISO.extract_isosurface(torch.from_numpy(values), bounds=BOUNDS, backend=BACKEND)
        _cache[("dense", kind, n)] = (v.numpy(), f.numpy())
    return _cache[("dense", kind, n)]


class CountingField:
    def __init__(self, kind, batch=1):
        self.kind, self.batch, self.calls = kind, batch, []

    def __call__(self, points):
        assert points.dim() == 3 and points.shape[0] == 1 and points.shape[2] == 3 and points.dtype == torch.float32
        self.calls.append(points.shape[1])
        p = points[0].numpy()
        val = torch.from_numpy(_field_f32(self.kind, p[:, 0], p[:, 1], p[:, 2]))
        return val.reshape(1, -1, 1).expand(self.batch, -1, -1)


@pytest.mark.parametrize("dilation", [0, 1])
@pytest.mark.parametrize("dense", [3, 4])
@pytest.mark.parametrize("kind", ["sphere", "torus"])
def test_hierarchy_equals_the_dense_extraction_bit_for_bit(kind, dense, dilation, caplog):
    field = CountingField(kind)
    with caplog.at_level(logging.WARNING, logger="actionmesh_amd.isosurface"):
        out = ISO.hierarchical_extract_geometry(field, "cpu", bounds=BOUNDS, dense_octree_depth=dense, hierarchical_octree_depth=5,
                                                dilation=dilation, backend=BACKEND)
    assert not caplog.records                                      # closed: no border warning
    assert len(out) == 1
    v, f = out[0]
    dv, df = _dense(kind, 33)
    assert isinstance(v, np.ndarray) and v.dtype == np.float32 and f.dtype == np.int64
    assert np.array_equal(v.view(np.uint32), dv.view(np.uint32)) and np.array_equal(f, df)
    dense_points = (2 ** dense + 1) ** 3
    assert field.calls[0] == dense_points
    finest = field.calls[-1]
    print(f"{kind} {dense} -> 5, dilation {dilation}: evaluated {field.calls}, {finest} of {33 ** 3} points at the finest depth")
    assert sum(field.calls) < 33 ** 3 and 0 < finest < 33 ** 3


def test_hierarchy_chunks_batches_and_warns_about_borders(caplog):
    field = CountingField("sphere", batch=2)
    out = ISO.hierarchical_extract_geometry(field, "cpu", bounds=BOUNDS, dense_octree_depth=3, hierarchical_octree_depth=4,
                                            max_points_per_call=500, backend=BACKEND)
    assert len(out) == 2 and max(field.calls) <= 500
    dv, df = _dense("sphere", 17)
    for v, f in out:
        assert np.array_equal(v.view(np.uint32), dv.view(np.uint32)) and np.array_equal(f, df)
    # a box the sphere leaves: an open surface, reported
    with caplog.at_level(logging.WARNING, logger="actionmesh_amd.isosurface"):
        (v, f), = ISO.hierarchical_extract_geometry(CountingField("sphere"), "cpu", bounds=0.7, dense_octree_depth=3,
                                                    hierarchical_octree_depth=4, backend=BACKEND)
    assert any("border edges" in r.getMessage() for r in caplog.records) and (R.edge_use_counts(f) == 1).any()
    # no further depth: the dense grid itself
    (v, f), = ISO.hierarchical_extract_geometry(CountingField("sphere"), "cpu", bounds=BOUNDS, dense_octree_depth=4,
                                                hierarchical_octree_depth=4, backend=BACKEND)
    assert np.array_equal(v.view(np.uint32), dv.view(np.uint32)) and np.array_equal(f, df)


# ---- chain ---------------------------------------------------------------------------------------------------------------------------
def test_chain_into_clean_up_and_decimation():
    import _decimate_ref as D
    from actionmesh_amd import mesh_decimate, mesh_prep
    v, f = extract("sphere", 17)
    cv, cf = mesh_prep.merge_and_clean_mesh(torch.from_numpy(v), torch.from_numpy(f))[:2]
    dv, df = mesh_decimate.decimate_mesh(cv, cf, 1000, backend=D.NumpyBackend())
    assert df.shape[0] == 1000
    R.check_closed_oriented(dv.numpy(), df.numpy(), 2)
    radius = np.linalg.norm(dv.double().numpy() - np.asarray(R.SPHERE_CENTRE), axis=1)
    print("decimated sphere: radius", radius.min(), "..", radius.max())
    assert 0.79 <= radius.min() and radius.max() <= 0.81


# ---- seam ----------------------------------------------------------------------------------------------------------------------------
def test_install_into_and_uninstall_from_a_stand_in_module(monkeypatch):
    pipeline = types.ModuleType(ISO.PIPELINE_MODULE)
    pipeline.hierarchical_extract_geometry = "triposg's own"
    for name in ("triposg", "triposg.pipelines"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        monkeypatch.setitem(sys.modules, name, pkg)
    monkeypatch.setitem(sys.modules, ISO.PIPELINE_MODULE, pipeline)
    mod = types.ModuleType("stand_in")
    mod.hierarchical_extract_geometry = "imported from triposg"
    saved = ISO.install_into(mod)
    assert mod.hierarchical_extract_geometry is ISO.hierarchical_extract_geometry is pipeline.hierarchical_extract_geometry
    ISO.uninstall_from(mod, saved)
    assert mod.hierarchical_extract_geometry == "imported from triposg" and pipeline.hierarchical_extract_geometry == "triposg's own"
    bare = types.ModuleType("bare")
    monkeypatch.delitem(sys.modules, ISO.PIPELINE_MODULE)
    ISO.uninstall_from(bare, ISO.install_into(bare))
    assert not hasattr(bare, "hierarchical_extract_geometry")


def test_signature_serves_the_reference_call_site():
    """triposg.py:193-199 calls (geometric_func, self.device, bounds=, dense_octree_depth=, hierarchical_octree_depth=)."""
    params = inspect.signature(ISO.hierarchical_extract_geometry).parameters
    assert list(params)[:5] == ["geometric_func", "device", "bounds", "dense_octree_depth", "hierarchical_octree_depth"]
    assert params["bounds"].default == (-1.005,) * 3 + (1.005,) * 3
    assert params["dense_octree_depth"].default == 8 and params["hierarchical_octree_depth"].default == 9


@pytest.fixture
def reference_triposg(monkeypatch):
    """The reference's own actionmesh.external.triposg, imported under stub `triposg`, `trimesh` and `diffusers` modules (none of
    them is installed where these tests run); every sys.modules entry made here is removed again."""
    if not HAVE_REF:
        pytest.skip("reference not present")

    class Trimesh:
        def __init__(self, vertices, faces):
            self.vertices, self.faces = vertices, faces

    class TripoSGVAEModel:
        def __init__(self, *a, **k):
            self.device = torch.device("cpu")

    def theirs(*a, **k):
        raise AssertionError("triposg's own hierarchical_extract_geometry was called")

    stubs = {}
    for name in ("triposg", "triposg.models", "triposg.pipelines", "diffusers"):
        stubs[name] = types.ModuleType(name)
        stubs[name].__path__ = []
    for name, attrs in (("trimesh", dict(Trimesh=Trimesh)), ("diffusers.image_processor", dict(PipelineImageInput=object)),
                        ("triposg.inference_utils", dict(hierarchical_extract_geometry=theirs)),
                        ("triposg.models.autoencoders", dict(TripoSGVAEModel=TripoSGVAEModel)),
                        ("triposg.pipelines.pipeline_triposg", dict(TripoSGPipeline=object, hierarchical_extract_geometry=theirs))):
        stubs[name] = types.ModuleType(name)
        for k, val in attrs.items():
            setattr(stubs[name], k, val)
    for name, mod in stubs.items():
        monkeypatch.setitem(sys.modules, name, mod)
    for name in [n for n in sys.modules if n == "actionmesh" or n.startswith("actionmesh.")]:
        monkeypatch.delitem(sys.modules, name)                     # an earlier test's import of the reference, made under other stubs
    before = set(sys.modules)
    monkeypatch.syspath_prepend(REF)
    try:
        yield importlib.import_module("actionmesh.external.triposg"), stubs, theirs
    finally:
        for name in set(sys.modules) - before:
            if name == "actionmesh" or name.startswith("actionmesh."):
                del sys.modules[name]


def test_the_references_decode_latents_reaches_the_installed_function(reference_triposg, monkeypatch):
    T, stubs, theirs = reference_triposg
    assert T.hierarchical_extract_geometry is theirs
    monkeypatch.setattr(ISO, "HipBackend", R.NumpyBackend)          # no device here: the restatement behind the installed function
    monkeypatch.setattr(T, "_is_pytorch3d_available", True)
    saved = ISO.install_into(T)
    try:
        assert stubs["triposg.pipelines.pipeline_triposg"].hierarchical_extract_geometry is ISO.hierarchical_extract_geometry
        vae = T.TripoSGVAE()
        field = CountingField("sphere")
        vae.decode = lambda latents, sampled_points: types.SimpleNamespace(sample=field(sampled_points))
        meshes = vae.decode_latents(torch.zeros(1, 4, 8), dense_octree_depth=3, hierarchical_octree_depth=4)
    finally:
        ISO.uninstall_from(T, saved)
    assert T.hierarchical_extract_geometry is theirs and stubs["triposg.pipelines.pipeline_triposg"].hierarchical_extract_geometry is theirs
    dv, df = _dense("sphere", 17)
    assert len(meshes) == 1 and np.array_equal(meshes[0].vertices, dv) and np.array_equal(meshes[0].faces, df)


def test_dropin_and_cli_switches_are_off_by_default():
    assert "isosurface" not in inspect.signature(dropin.install).parameters          # a call of its own, like install_preprocess()
    assert callable(dropin.install_isosurface)
    assert cli.split_args([])[0].isosurface == "off"
    ours, rest = cli.split_args(["--isosurface", "hip", "--", "--fast"])
    assert ours.isosurface == "hip" and rest == ["--fast"]
