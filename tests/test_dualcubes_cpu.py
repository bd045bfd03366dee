"""Dual marching cubes without a device: the shipped Python (actionmesh_amd/isosurface.py, method="dual") on CPU tensors, with the
numpy restatement of the header's contract (tests/_dualcubes_ref.py) in place of the kernels.

* the tables the restatement derives from the header's rule: the patch-count histogram, the 36 configurations with a double face;
* the smallest tunnel, where exactly one face flips, and its complement, where none does;
* white noise (flips next to each other) and its smoothing: every edge in two faces, every directed edge once, every vertex's link one
  cycle, every vertex used - and what the default rule alone would give;
* the analytic fields of tests/_isosurface_ref.py: the same invariants with the Euler characteristic, orientation, the other
  comparison on the negated field, the triangle count against marching tetrahedra, the enclosed volume;
* non-finite samples, border edges, dropped vertices; the hierarchy against the dense extraction; the chain into
  `merge_and_clean_mesh` and `decimate_mesh`; the arguments, the drop-in and the command line.
The figures are the contract's, measured on a prototype that follows the same rules - not the code under test's.
"""
import inspect
import logging
import types

import numpy as np
import pytest
import torch

import _dualcubes_ref as D
import _isosurface_ref as R
from actionmesh_amd import cli, dropin
from actionmesh_amd import isosurface as ISO

BACKENDS = dict(backend=R.NumpyBackend(), dual_backend=D.NumpyBackend())
FIELDS = {"sphere": R.sphere, "torus": R.torus, "two_spheres": R.two_spheres}
_cache = {}


def extract(name, n=None, method="dual"):
    """The shipped wrapper on one of the fields, once per case: (vertices, faces) as numpy arrays."""
    if (name, n, method) not in _cache:
        if name == "octahedron":
            values, frame = R.octahedron(), {}
        else:
            values, frame = FIELDS[name](n), dict(zip(("origin", "spacing"), R.frame(n)))
        v, f = ISO.extract_isosurface(torch.from_numpy(values), method=method, **frame, **BACKENDS)
        assert v.dtype == torch.float32 and f.dtype == torch.int64 and v.shape[1:] == (3,) and f.shape[1:] == (3,)
        _cache[(name, n, method)] = (v.numpy(), f.numpy())
    return _cache[(name, n, method)]


def dual(values, **kwargs):
    v, f = ISO.extract_isosurface(torch.from_numpy(values), method="dual", **kwargs, **BACKENDS)
    return v.numpy(), f.numpy()


def same_mesh(got, want):
    return (got[0].dtype == np.float32 and got[0].shape == want[0].shape and got[1].shape == want[1].shape
            and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1]))


def components(n_vertices, faces):
    """The number of connected components of the mesh."""
    label = np.arange(n_vertices)
    while True:
        low = label.copy()
        for a, b in ((0, 1), (1, 2), (2, 0)):
            np.minimum.at(low, faces[:, a], label[faces[:, b]])
        low = low[low]
        if np.array_equal(low, label):
            return np.unique(label).shape[0]
        label = low


# ---- tables ----------------------------------------------------------------------------------------------------------------------------
def test_the_restatement_derives_the_tables_it_uses():
    assert np.bincount(D.NPATCH[0], minlength=5).tolist() == [2, 162, 82, 8, 2]
    with_double = np.nonzero(D.DOUBLE)[0]
    assert with_double.shape[0] == 36
    for cfg in with_double:
        assert bin(int(D.AMBIGUOUS[cfg])).count("1") == 1 and D.DOUBLE[cfg] == D.AMBIGUOUS[cfg]      # exactly one ambiguous face: the double one
        assert not np.array_equal(D.PATCH[0, cfg], D.PATCH[1, cfg])
    without = np.nonzero(D.DOUBLE == 0)[0]
    assert np.array_equal(D.PATCH[0, without], D.PATCH[1, without])
    assert D.EDGES == [(0, 1), (0, 2), (0, 4), (1, 3), (1, 5), (2, 3), (2, 6), (3, 7), (4, 5), (4, 6), (5, 7), (6, 7)]
    for flip in range(2):
        for cfg in range(256):
            crossing = np.array([(cfg >> a & 1) != (cfg >> b & 1) for a, b in D.EDGES])
            assert np.array_equal(D.PATCH[flip, cfg] != 255, crossing)                                  # every crossing edge on a patch
            patches = D.PATCH[flip, cfg][crossing]
            assert sorted(set(patches.tolist())) == list(range(D.NPATCH[flip, cfg]))
            first = [int(np.nonzero(D.PATCH[flip, cfg] == q)[0][0]) for q in range(D.NPATCH[flip, cfg])]
            assert first == sorted(first)                                                               # numbered by smallest edge
            assert all((D.PATCH[flip, cfg] == q).sum() >= 3 for q in range(D.NPATCH[flip, cfg]))
    # the complement of a configuration crosses the same edges; a double face belongs to the six-inside side of a two-corner diagonal
    assert np.array_equal(D.PATCH[0] != 255, D.PATCH[0, ::-1] != 255)


# ---- the smallest tunnel ---------------------------------------------------------------------------------------------------------------
def tunnel(sign):
    values = np.full((4, 4, 4), sign, dtype=np.float32)
    values[1, 2, 2] = values[2, 1, 2] = -sign
    return values


@pytest.mark.parametrize("sign, flips", [(1.0, 1), (-1.0, 0)])
def test_the_smallest_tunnel_and_its_complement(sign, flips):
    """All inside but two points diagonal on one cell face: the two cells that share the face see a tunnel each by the default rule
    (double on both sides), the flip separates the two outside points.  The complement has two inside points, no double face."""
    values = tunnel(sign)
    assert D.flipped_faces(values) == flips
    v, f = dual(values)
    assert (v.shape[0], f.shape[0]) == (16, 24) and components(16, f) == 2
    D.check_manifold(v, f, 4)
    assert (R.edge_use_counts(f) == 2).all()
    assert same_mesh((v, f), D.ref_extract(values))


# ---- white noise -----------------------------------------------------------------------------------------------------------------------
def noise_fields():
    """Prototype field #0 and its smoothing with sigma = 1 (a truncated separable Gaussian), the six border planes at -1."""
    if "noise" not in _cache:
        def closed(a):
            a = a.copy()
            for s in (0, -1):
                a[s], a[:, s], a[:, :, s] = -1.0, -1.0, -1.0
            return a.astype(np.float32)
        raw = closed(np.random.default_rng(0).standard_normal((21, 21, 21)))
        x = np.arange(-4, 5)
        kernel = np.exp(-0.5 * x ** 2.0)
        kernel /= kernel.sum()
        smooth = raw.astype(np.float64)
        for axis in range(3):
            smooth = np.apply_along_axis(lambda line: np.convolve(np.pad(line, 4, mode="edge"), kernel, mode="valid"), axis, smooth)
        _cache["noise"] = {"raw": raw, "smooth": closed(smooth)}
    return _cache["noise"]


@pytest.mark.parametrize("which", ["raw", "smooth"])
def test_white_noise_is_a_closed_manifold(which):
    values = noise_fields()[which]
    flips = D.flipped_faces(values)
    v, f = dual(values)
    print(f"noise {which}: {v.shape[0]} vertices, {f.shape[0]} triangles, {flips} flipped faces")
    assert f.shape[0] > 200
    if which == "raw":
        assert flips > 0                                           # 84 in the prototype: the path is exercised
    D.check_manifold(v, f)
    assert same_mesh((v, f), D.ref_extract(values))


def test_without_the_flip_white_noise_is_not_a_manifold():
    """What the rule is for: on the same field the default rule alone leaves edges in four faces and vertices whose link is two
    cycles (84 and 168 in the prototype)."""
    values = noise_fields()["raw"]
    v, f = D.ref_extract_without_flips(values)
    crowded, pinched = D.edges_in_more_than_two_faces(f), len(D.vertices_whose_link_is_not_one_cycle(v.shape[0], f))
    print("without flips:", crowded, "edges in more than two faces,", pinched, "vertices whose link is not one cycle")
    assert crowded > 0 and pinched > 0


# ---- analytic fields -------------------------------------------------------------------------------------------------------------------
CASES = [("sphere", 9, 2), ("sphere", 17, 2), ("sphere", 33, 2), ("torus", 17, 0), ("torus", 33, 0), ("two_spheres", 17, 4),
         ("octahedron", None, 2)]


@pytest.mark.parametrize("name, n, chi", CASES)
def test_closed_oriented_manifold_with_its_euler_characteristic(name, n, chi):
    v, f = extract(name, n)
    D.check_manifold(v, f, chi)
    assert R.signed_volume(v, f) > 0 and f.shape[0] % 2 == 0
    if name == "two_spheres":
        assert components(v.shape[0], f) == 2


def test_normals_point_down_the_gradient():
    v, f = extract("sphere", 17)
    normal, area = R.face_normals_and_areas(v, f)
    assert (area >= 1e-12).all()
    outward = v.astype(np.float64)[f].mean(axis=1) - np.asarray(R.SPHERE_CENTRE)
    assert (np.einsum("ij,ij->i", normal, outward) > 0).all()
    v, f = extract("octahedron")
    normal, area = R.face_normals_and_areas(v, f)
    keep = area >= 1e-12
    print("octahedron: degenerate faces", int((~keep).sum()), "of", f.shape[0])
    centroid = v.astype(np.float64)[f].mean(axis=1) - 4.0
    assert keep.any() and (np.einsum("ij,ij->i", normal, np.sign(centroid))[keep] > 0).all()


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_inside_below_on_the_negated_field_is_the_identical_mesh(name):
    o, s = R.frame(17)
    got = dual(-FIELDS[name](17), origin=o, spacing=s, inside="below")
    assert same_mesh(got, extract(name, 17))
    # and the other side of the same values is a closed surface with the reverse winding
    rv, rf = dual(FIELDS[name](17), origin=o, spacing=s, inside="below")
    assert R.signed_volume(rv, rf) < 0
    D.check_manifold(rv, rf)


@pytest.mark.parametrize("n", [9, 17, 33])
def test_fewer_than_half_the_triangles_of_marching_tetrahedra(n):
    d, t = extract("sphere", n)[1].shape[0], extract("sphere", n, "tetrahedra")[1].shape[0]
    print(f"sphere {n}^3: {d} triangles against {t}: {d / t:.3f}")
    assert d < 0.5 * t


def test_volume_rises_with_the_resolution():
    """The mean of a patch's crossings lies inside a convex surface, so the enclosed volume is below the analytic one and rises
    towards it.  Measured on the restatement: sphere 9^3 / 17^3 / 33^3 0.8970 / 0.9739 / 0.9934, torus 17^3 / 33^3 0.8997 / 0.9768
    (the device adds nothing: it is bit-identical)."""
    sphere = [R.signed_volume(*extract("sphere", n)) / R.SPHERE_VOLUME for n in (9, 17, 33)]
    torus = [R.signed_volume(*extract("torus", n)) / R.TORUS_VOLUME for n in (17, 33)]
    print("volume / analytic: sphere", sphere, "torus", torus)
    assert sphere[0] < sphere[1] < sphere[2] < 1 and torus[0] < torus[1] < 1


# ---- non-finite samples, borders --------------------------------------------------------------------------------------------------------
def test_non_finite_samples_open_the_surface_and_unused_vertices_are_dropped():
    r = np.random.default_rng(0).standard_normal((9, 9, 9)).astype(np.float32)
    r[2, 3, 4], r[5, 5, 1], r[6, 2, 6] = np.nan, np.inf, -np.inf
    v, f = dual(r)
    uses = R.edge_use_counts(f)
    assert (uses <= 2).all() and (uses == 1).any() and R.directed_edges_unique(f) and R.all_vertices_used(v.shape[0], f)
    assert ISO.border_edge_count(torch.from_numpy(f)) == int((uses == 1).sum())
    # no triangle touches a cell with a non-finite corner: a dual vertex lies inside its cell (index frame, no exact hits here)
    cell = np.floor(v.astype(np.float64)).astype(np.int64)
    assert (cell >= 0).all() and (cell <= 7).all()
    finite = np.isfinite(r)
    for m in range(8):
        assert finite[cell[:, 0] + (m >> 2 & 1), cell[:, 1] + (m >> 1 & 1), cell[:, 2] + (m & 1)].all()
    # the restatement without the wrapper's compaction has vertices that no face uses; the wrapper dropped them, order preserved
    rv, rf = D.ref_extract(r, compact=False)
    assert np.unique(rf).shape[0] == v.shape[0] < rv.shape[0]
    assert np.array_equal(rv[np.unique(rf)].view(np.uint32), v.view(np.uint32))


def test_surface_cut_by_the_grid_border_is_open():
    x, y, z = R.axes(9)
    values = R.sphere_of(x, y, z, 1.2, (0, 0, 0)).astype(np.float32)
    v, f = dual(values, bounds=(-1,) * 3 + (1,) * 3)
    uses = R.edge_use_counts(f)
    assert f.shape[0] > 0 and (uses == 1).any() and (uses <= 2).all()
    assert ISO.border_edge_count(torch.from_numpy(f)) == int((uses == 1).sum())
    assert float(np.abs(v).max()) < 1.0


def test_noncubic_anisotropic_and_a_level_equal_the_restatement():
    values, origin, spacing = R.noncubic_with_nans()
    got = dual(values, origin=origin, spacing=spacing)
    assert got[1].shape[0] > 150 and same_mesh(got, D.ref_extract(values, 0.0, origin, spacing))
    assert same_mesh(dual(values, level=0.25, origin=origin, spacing=spacing), D.ref_extract(values, 0.25, origin, spacing))


@pytest.mark.parametrize("fill", [1.0, -1.0, float("nan")])
def test_grids_without_a_crossing_are_empty(fill):
    v, f = ISO.extract_isosurface(torch.full((5, 6, 7), fill), method="dual", **BACKENDS)
    assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == torch.float32 and f.dtype == torch.int64


def test_one_cell_has_vertices_and_no_quad():
    values = torch.full((2, 2, 2), -1.0)
    values[0, 0, 0] = 1.0
    v, f = ISO.extract_isosurface(values, method="dual", **BACKENDS)
    assert v.shape == (0, 3) and f.shape == (0, 3)                 # a quad needs the four cells around an edge


# ---- hierarchy -------------------------------------------------------------------------------------------------------------------------
BOUNDS = (-1.005,) * 3 + (1.005,) * 3


def _field_f32(kind, x, y, z):
    if kind == "sphere":
        return (0.8 - np.sqrt((x - 0.03) ** 2 + (y + 0.02) ** 2 + (z - 0.01) ** 2)).astype(np.float32)
    return (0.25 - np.sqrt((np.sqrt(x ** 2 + y ** 2) - 0.6) ** 2 + z ** 2)).astype(np.float32)


def _dense(kind, n):
    if ("dense", kind, n) not in _cache:
        x = np.linspace(-1.005, 1.005, n).astype(np.float32)
        _cache[("dense", kind, n)] = dual(_field_f32(kind, *np.meshgrid(x, x, x, indexing="ij")), bounds=BOUNDS)
    return _cache[("dense", kind, n)]


class CountingField:
    def __init__(self, kind):
        self.kind, self.calls = kind, []

    def __call__(self, points):
        assert points.dim() == 3 and points.shape[0] == 1 and points.shape[2] == 3 and points.dtype == torch.float32
        self.calls.append(points.shape[1])
        p = points[0].numpy()
        return torch.from_numpy(_field_f32(self.kind, p[:, 0], p[:, 1], p[:, 2])).reshape(1, -1, 1)


@pytest.mark.parametrize("dense", [3, 4])
@pytest.mark.parametrize("kind", ["sphere", "torus"])
def test_hierarchy_equals_the_dense_extraction_bit_for_bit(kind, dense, caplog):
    field = CountingField(kind)
    with caplog.at_level(logging.WARNING, logger="actionmesh_amd.isosurface"):
        (v, f), = ISO.hierarchical_extract_geometry(field, "cpu", bounds=BOUNDS, dense_octree_depth=dense, hierarchical_octree_depth=5,
                                                    method="dual", **BACKENDS)
    assert not caplog.records                                      # closed: no border warning
    assert isinstance(v, np.ndarray) and f.dtype == np.int64 and same_mesh((v, f), _dense(kind, 33))
    assert field.calls[0] == (2 ** dense + 1) ** 3 and sum(field.calls) < 33 ** 3
    D.check_manifold(v, f, {"sphere": 2, "torus": 0}[kind])


# ---- chain -----------------------------------------------------------------------------------------------------------------------------
def test_chain_into_clean_up_and_decimation():
    import _decimate_ref
    from actionmesh_amd import mesh_decimate, mesh_prep
    v, f = extract("sphere", 33)
    assert f.shape[0] > 2000
    cv, cf = mesh_prep.merge_and_clean_mesh(torch.from_numpy(v), torch.from_numpy(f))[:2]
    dv, df = mesh_decimate.decimate_mesh(cv, cf, 2000, backend=_decimate_ref.NumpyBackend())
    assert df.shape[0] == 2000
    R.check_closed_oriented(dv.numpy(), df.numpy(), 2)


# ---- arguments and switches ------------------------------------------------------------------------------------------------------------
def test_method_argument():
    values = torch.from_numpy(R.sphere(9))
    for call in (lambda m: ISO.extract_isosurface(values, method=m, **BACKENDS),
                 lambda m: ISO.hierarchical_extract_geometry(CountingField("sphere"), "cpu", dense_octree_depth=3,
                                                             hierarchical_octree_depth=3, method=m, **BACKENDS)):
        with pytest.raises(ValueError, match="method"):
            call("cubes")
    for m in ("cubes", None):
        with pytest.raises(ValueError, match="method"):
            ISO.install_into(types.ModuleType("stand_in"), method=m)
    with pytest.raises(ValueError, match="method"):
        dropin.install_isosurface(method="cubes")
    default = ISO.extract_isosurface(values, **BACKENDS)
    named = ISO.extract_isosurface(values, method="tetrahedra", **BACKENDS)
    assert torch.equal(default[0], named[0]) and torch.equal(default[1], named[1])
    other = ISO.extract_isosurface(values, method="dual", **BACKENDS)
    assert other[1].shape[0] < named[1].shape[0]
    with pytest.raises(RuntimeError):                              # no CPU path: the shipped backend refuses a CPU tensor
        ISO.extract_isosurface(values, method="dual")
    assert inspect.signature(ISO.extract_isosurface).parameters["method"].default == "tetrahedra"
    assert inspect.signature(ISO.hierarchical_extract_geometry).parameters["method"].default == "tetrahedra"


def test_install_into_with_the_dual_method():
    mod = types.ModuleType("stand_in")
    mod.hierarchical_extract_geometry = "imported from triposg"
    saved = ISO.install_into(mod, method="dual")
    assert mod.hierarchical_extract_geometry is ISO.hierarchical_extract_geometry_dual
    (v, f), = mod.hierarchical_extract_geometry(CountingField("sphere"), "cpu", bounds=BOUNDS, dense_octree_depth=3,
                                                hierarchical_octree_depth=4, **BACKENDS)
    assert same_mesh((v, f), _dense("sphere", 17))
    ISO.uninstall_from(mod, saved)
    assert mod.hierarchical_extract_geometry == "imported from triposg"
    ISO.uninstall_from(mod, ISO.install_into(mod))
    assert mod.hierarchical_extract_geometry == "imported from triposg"


def test_dropin_and_cli_switches():
    assert inspect.signature(dropin.install_isosurface).parameters["method"].default == "tetrahedra"
    assert cli.split_args([])[0].isosurface == "off"
    ours, rest = cli.split_args(["--isosurface", "hip-dual", "--", "--fast"])
    assert ours.isosurface == "hip-dual" and rest == ["--fast"]
    from actionmesh_amd import ops
    assert ops.dmc_flag_message(1 | 4).count(";") == 1 and "code" in ops.dmc_flag_message(4) and "triangle" in ops.dmc_flag_message(2)
