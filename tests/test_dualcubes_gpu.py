"""Dual marching cubes on the device (actionmesh_amd/isosurface.py, method="dual", over csrc/am_dualcubes.hip) against the numpy
restatement of the header (tests/_dualcubes_ref.py), bit for bit: the whole extraction, run twice; the edge cases; the hierarchy
against the dense grid with an analytic field evaluated on the device; and the chain into the device's clean-up and decimation.  The
kernels one by one, inside guard bands, are tests/test_guard_dualcubes_gpu.py's."""
import logging

import numpy as np
import pytest
import torch

import _dualcubes_ref as D
import _isosurface_ref as R

pytestmark = pytest.mark.gpu

BOUNDS = (-1.005,) * 3 + (1.005,) * 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from actionmesh_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def same_mesh(got, want):
    (gv, gf), (wv, wf) = got, want
    gv, gf = (t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in (gv, gf))
    return (gv.dtype == np.float32 and gf.dtype == np.int64 and gv.shape == wv.shape and gf.shape == wf.shape
            and np.array_equal(gv.view(np.uint32), wv.view(np.uint32)) and np.array_equal(gf, wf))


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_whole_extraction_equals_the_restatement_twice(dev, name):
    from actionmesh_amd import isosurface as ISO
    values = {"sphere": R.sphere, "torus": R.torus}[name](33)
    origin, spacing = R.frame(33)
    want = D.ref_extract(values, 0.0, origin, spacing)
    assert want[1].shape[0] > 4000
    t = torch.from_numpy(values).to(dev)
    for _ in range(2):
        got = ISO.extract_isosurface(t, origin=origin, spacing=spacing, method="dual")
        assert got[0].device.type == "cuda" and got[1].device.type == "cuda" and same_mesh(got, want)
    D.check_manifold(want[0], want[1], {"sphere": 2, "torus": 0}[name])


def test_edge_cases_equal_the_restatement(dev):
    from actionmesh_amd import isosurface as ISO
    # non-cubic, anisotropic, non-finite samples
    values, origin, spacing = R.noncubic_with_nans()
    got = ISO.extract_isosurface(torch.from_numpy(values).to(dev), origin=origin, spacing=spacing, method="dual")
    assert same_mesh(got, D.ref_extract(values, 0.0, origin, spacing))
    # exact hits
    assert same_mesh(ISO.extract_isosurface(torch.from_numpy(R.octahedron()).to(dev), method="dual"), D.ref_extract(R.octahedron()))
    # the other comparison on the negated field: the identical mesh
    values = R.sphere(17)
    origin, spacing = R.frame(17)
    want = D.ref_extract(values, 0.0, origin, spacing)
    assert same_mesh(ISO.extract_isosurface(torch.from_numpy(-values).to(dev), origin=origin, spacing=spacing, inside="below", method="dual"),
                     want)
    # white noise: faces that flip next to each other; a closed manifold all the same
    noise = np.random.default_rng(0).standard_normal((21, 21, 21))
    for s in (0, -1):
        noise[s], noise[:, s], noise[:, :, s] = -1.0, -1.0, -1.0
    noise = noise.astype(np.float32)
    assert D.flipped_faces(noise) > 0
    got = ISO.extract_isosurface(torch.from_numpy(noise).to(dev), method="dual")
    assert same_mesh(got, D.ref_extract(noise))
    D.check_manifold(got[0].cpu().numpy(), got[1].cpu().numpy())
    # a random field with samples not evaluated: open, never more than two faces on an edge, unused vertices dropped
    r = np.random.default_rng(0).standard_normal((9, 9, 9)).astype(np.float32)
    r[2, 3, 4] = r[5, 5, 1] = np.nan
    got = ISO.extract_isosurface(torch.from_numpy(r).to(dev), method="dual")
    assert same_mesh(got, D.ref_extract(r)) and (R.edge_use_counts(got[1].cpu().numpy()) <= 2).all()
    assert got[0].shape[0] < D.ref_extract(r, compact=False)[0].shape[0]
    # the smallest grid (vertices, no quad) and grids without a crossing
    small = np.full((2, 2, 2), -1.0, dtype=np.float32)
    small[1, 0, 1] = 2.0
    for t in (torch.from_numpy(small).to(dev),) + tuple(torch.full((5, 6, 7), fill, device=dev) for fill in (1.0, -1.0, float("nan"))):
        v, f = ISO.extract_isosurface(t, method="dual")
        assert v.shape == (0, 3) and f.shape == (0, 3) and v.device.type == "cuda"


def test_a_tile_boundary_on_every_axis(dev):
    """21 x 13 x 70 points: more than one am_dmc_cells tile along every axis (8 x 8 x 64 points each), none of them full."""
    from actionmesh_amd import isosurface as ISO
    i, j, k = np.meshgrid(np.arange(21), np.arange(13), np.arange(70), indexing="ij")
    values = (np.sin(0.45 * i + 0.2) * np.cos(0.6 * j) + np.sin(0.31 * k - 0.4) * 0.8).astype(np.float32)
    values[7, 8, 63], values[8, 7, 64] = np.nan, np.nan            # next to the tile corners
    spacing = (0.5, 1.25, 0.75)
    got = ISO.extract_isosurface(torch.from_numpy(values).to(dev), level=0.1, origin=(1.0, -2.0, 0.5), spacing=spacing, method="dual")
    want = D.ref_extract(values, 0.1, (1.0, -2.0, 0.5), spacing)
    assert want[1].shape[0] > 1500 and same_mesh(got, want)


def _sphere_on_device(points):
    x, y, z = points[..., 0], points[..., 1], points[..., 2]
    return (0.8 - torch.sqrt((x - 0.03) ** 2 + (y + 0.02) ** 2 + (z - 0.01) ** 2)).unsqueeze(-1)


def test_hierarchy_equals_the_dense_extraction(dev, caplog):
    from actionmesh_amd import isosurface as ISO
    calls = []

    def field(points):
        assert points.device.type == "cuda" and points.shape[0] == 1 and points.dtype == torch.float32
        calls.append(points.shape[1])
        return _sphere_on_device(points)

    with caplog.at_level(logging.WARNING, logger="actionmesh_amd.isosurface"):
        (v, f), = ISO.hierarchical_extract_geometry(field, dev, bounds=BOUNDS, dense_octree_depth=4, hierarchical_octree_depth=6,
                                                    method="dual")
    assert not caplog.records
    axis = ISO._axis_points(-1.005, 1.005, 65, dev)
    grid = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), dim=-1).reshape(1, -1, 3)
    dense = _sphere_on_device(grid).reshape(65, 65, 65)
    want = D.ref_extract(dense.cpu().numpy(), 0.0, (-1.005,) * 3, ((1.005 + 1.005) / 64,) * 3)
    assert same_mesh((v, f), want) and same_mesh(ISO.extract_isosurface(dense, bounds=BOUNDS, method="dual"), want)
    D.check_manifold(v, f, 2)
    assert calls[0] == 17 ** 3 and sum(calls) < 65 ** 3


def test_chain_into_clean_up_and_decimation(dev):
    from actionmesh_amd import isosurface as ISO, mesh_decimate, mesh_prep
    origin, spacing = R.frame(33)
    v, f = ISO.extract_isosurface(torch.from_numpy(R.sphere(33)).to(dev), origin=origin, spacing=spacing, method="dual")
    cv, cf = mesh_prep.merge_and_clean_mesh(v, f)[:2]
    dv, df = mesh_decimate.decimate_mesh(cv, cf, 2000)
    assert df.shape[0] == 2000 and dv.device.type == "cuda"
    R.check_closed_oriented(dv.cpu().numpy(), df.cpu().numpy(), 2)
    radius = np.linalg.norm(dv.double().cpu().numpy() - np.asarray(R.SPHERE_CENTRE), axis=1)
    print("decimated sphere: radius", radius.min(), "..", radius.max())
