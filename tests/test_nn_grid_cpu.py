"""The grid nearest-neighbour search without a GPU: the numpy restatement of the header's build and ring walk (tests/_nn_grid_ref.py)
against a numpy brute force (am_nn_search's contract) in both precisions and against scipy's cKDTree in fp64, on EVERY query of
every case; the gold fixture's neighbours; the C ABI's argument checks."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import _nn_grid_ref as R
from actionmesh_amd import _lib as L
from actionmesh_amd import ops

GOLD = os.path.join(os.path.dirname(__file__), "golden", "actionbench.npz")
F32 = np.float32


def _lattice():
    ax = np.arange(9, dtype=F32)
    pts = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    pts = pts[np.random.RandomState(1).permutation(len(pts))]          # the lowest index of eight tied corners is not the first in space
    h = np.arange(8, dtype=F32) + F32(0.5)
    return pts, np.stack(np.meshgrid(h, h, h, indexing="ij"), -1).reshape(-1, 3)


def cases():
    """name -> (points (P, 3), queries (Q, 3), cells per axis to try); None = the default"""
    rng = np.random.RandomState(7)
    out = {}
    cloud = rng.randn(400, 3).astype(F32)
    qry = (cloud[rng.permutation(400)[:150]] + 0.05 * rng.randn(150, 3)).astype(F32)
    out["one_point"] = (F32([[0.25, -1.0, 2.0]]), rng.randn(9, 3).astype(F32), [None, 1, 5])
    out["identical"] = (np.tile(F32([[1.5, -2.0, 0.125]]), (40, 1)), rng.randn(20, 3).astype(F32), [None, 3])
    flat = cloud.copy()
    flat[:, 2] = F32(0.75)
    out["flat"] = (flat, qry, [None, 7])
    out["lattice"] = _lattice() + ([None, 8, 9],)
    dup = cloud.copy()
    dup[200:300] = dup[:100]
    out["duplicates"] = (dup, np.concatenate([dup[250:300], qry]), [None])
    bad = cloud.copy()
    bad[5, 0], bad[17, 1], bad[33, 2], bad[34] = np.nan, np.inf, -np.inf, np.nan
    bq = qry.copy()
    bq[3, 0], bq[4, 2], bq[5, 1] = np.nan, np.inf, -np.inf
    out["non_finite"] = (bad, bq, [None, 4])
    far = np.concatenate([qry * F32(1e4), F32([[1e6, 0, 0], [-1e6, -1e6, -1e6], [0, 3e5, -2e5], [50, 50, 50]])])
    out["far_queries"] = (cloud, far, [None, 6])
    huge = (rng.rand(60, 3).astype(F32) * 2 - 1) * F32(3e38)
    out["huge"] = (huge, np.concatenate([huge[:10], (rng.rand(10, 3).astype(F32) * 2 - 1) * F32(3e38), rng.randn(5, 3).astype(F32)]), [None, 4])
    den = np.zeros((50, 3), dtype=F32)
    den[:, 0] = (np.arange(50) % 5).astype(F32) * F32(1e-45)            # extent 4 denormals: G / extent overflows, inv = 0
    den[:, 1] = rng.randn(50).astype(F32)
    out["denormal_extent"] = (den, np.concatenate([den[:20], rng.randn(10, 3).astype(F32)]), [None, 3])
    out["cells_1_2_many"] = (cloud[:7], qry[:40], [1, 2, 16, 128])       # G = 1, G = 2, G far larger than P
    out["cloud"] = (cloud, qry, [None, 5, 13])
    return out


CASES = cases()
RUNS = [(name, g) for name, (_, _, gs) in CASES.items() for g in gs]


@pytest.mark.parametrize("name,G", RUNS, ids=[f"{n}-G{g or 'default'}" for n, g in RUNS])
def test_restatement_equals_brute_force_and_kdtree(name, G):
    pts, qry, _ = CASES[name]
    G = R.default_cells(len(pts)) if G is None else G
    grid = R.build(pts, G)
    assert grid["cell_start"][0] == 0 and grid["cell_start"][-1] == len(pts) and (np.diff(grid["cell_start"]) >= 0).all()
    assert np.array_equal(np.sort(grid["order"]), np.arange(len(pts)))
    for dtype in (np.float32, np.float64):
        gi, gd = R.search(grid, qry, dtype)
        bi, bd = R.brute(pts, qry, dtype)
        assert np.array_equal(gi, bi), (name, dtype, np.nonzero(gi != bi)[0][:8])
        assert np.array_equal(gd.view(np.uint8), bd.view(np.uint8)), (name, dtype)
    # scipy's exact KD-tree, fp64, over the finite points (it rejects the others); every finite query
    fin_p, fin_q = np.isfinite(pts).all(1), np.isfinite(qry).all(1)
    assert (gi[~fin_q] == -1).all() and np.isinf(gd[~fin_q]).all()
    kd, ki = cKDTree(pts[fin_p].astype(np.float64)).query(qry[fin_q].astype(np.float64))
    ki = np.nonzero(fin_p)[0][ki]
    ours_i, ours_d = gi[fin_q], gd[fin_q]
    assert (ours_i >= 0).all()
    assert np.array_equal(np.sqrt(ours_d), kd), name                    # the same distance on every query
    d = qry[fin_q].astype(np.float64) - pts[ki].astype(np.float64)       # the tree's neighbour is one of the minimisers ...
    assert np.array_equal((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], ours_d)
    assert (ours_i <= ki).all()                                           # ... and ours is the lowest-index one


@pytest.mark.parametrize("name,G", RUNS, ids=[f"{n}-G{g or 'default'}" for n, g in RUNS])
def test_one_cell_function_gives_the_point_form(name, G):
    """the cell of a cloud's own point was min(G - 1, floor(t)) clamped at 0 (kept here as the thing compared against); the single
    clamped form gives the same cell for every finite point of every case"""
    pts = CASES[name][0]
    G = R.default_cells(len(pts)) if G is None else G
    frame = R.build(pts, G)["frame"]
    p = pts[np.isfinite(pts).all(axis=1)]
    old = np.zeros(p.shape, dtype=np.int64)
    with np.errstate(all="ignore"):
        for k in range(3):
            if frame[4 + k] != 0:
                t = ((p[:, k] - frame[k]).astype(F32) * frame[4 + k]).astype(F32)
                old[:, k] = np.maximum(0, np.minimum(G - 1, np.floor(t.astype(np.float64)).astype(np.int64)))
    assert len(p) and np.array_equal(R.cell_axes(p, frame, G), old)


def test_lattice_ties_go_to_the_lowest_index():
    pts, qry, _ = CASES["lattice"]
    grid = R.build(pts, 9)
    gi, gd = R.search(grid, qry, np.float32)
    assert (gd == F32(0.75)).all()
    d2 = ((qry[:, None, :] - pts[None]) ** 2).sum(-1)
    tied = d2 == 0.75
    assert (tied.sum(1) == 8).all() and np.array_equal(gi, tied.argmax(1))


def test_default_cells():
    for P, G in ((1, 2), (4, 2), (5, 3), (10_000, 28), (100_000, 59), (2_000_000, 128)):
        assert R.default_cells(P) == G == ops.nn_grid_default_cells(P)


def test_walk_evaluates_few_candidates_on_close_clouds():
    """what the grid is for: on surface samples queried by nearby points the walk touches a small part of the cloud"""
    rng = np.random.RandomState(3)
    u = rng.randn(3000, 3)
    pts = (u / np.linalg.norm(u, axis=1, keepdims=True) * [1.0, 0.7, 0.4]).astype(F32)
    count = []
    gi, _ = R.search(R.build(pts, R.default_cells(len(pts))), pts[:200] + F32(0.001), np.float32, count=count)
    assert np.array_equal(gi, R.brute(pts, pts[:200] + F32(0.001), np.float32)[0])
    assert np.mean(count) < 0.05 * len(pts), np.mean(count)


def test_gold_fixture_neighbours():
    gold = np.load(GOLD)
    for pts, qry, idx, dist in ((gold["preds"][0], gold["gts"][0], gold["nn_idx_gt_to_pred"], gold["nn_dist_gt_to_pred"]),
                                (gold["gts"][0], gold["preds"][0], gold["nn_idx_pred_to_gt"], gold["nn_dist_pred_to_gt"])):
        gi, gd = R.search(R.build(pts, R.default_cells(len(pts))), qry, np.float64)
        assert np.array_equal(gi, idx) and np.array_equal(np.sqrt(gd), dist)


def test_argument_validation_without_gpu():
    lib = L.lib()
    assert lib.am_nn_grid_cells(None, None) != 0 and b"null" in lib.am_last_error()
    assert lib.am_nn_grid_build(None, None) != 0 and b"null" in lib.am_last_error()
    assert lib.am_nn_grid_search(None, None) != 0 and b"null" in lib.am_last_error()
    assert lib.am_nn_grid_bytes(0, 1, 4) == 0 and lib.am_nn_grid_bytes(10, 1, 0) == 0 and lib.am_nn_grid_bytes(10, 1, 129) == 0
    assert lib.am_nn_grid_workspace_bytes(10, 0, 4) == 0
    # frame 32, slabs 6 * 4 * 4 = 96, cell_start (64 + 2) * 4 = 264 -> 272, order 40 -> 48, sorted 160
    assert lib.am_nn_grid_bytes(10, 1, 4) == 32 + 96 + 272 + 48 + 160
    assert lib.am_nn_grid_workspace_bytes(10, 3, 4) == 3 * (8 + 24) * 4 + 128          # extrema words, then 3 x 10 staged cells padded
    a = L.AmNnGridBuildArgs()
    a.grid.n_points, a.grid.batch, a.grid.cells = 10, 1, 200
    assert lib.am_nn_grid_cells(C.byref(a), None) != 0 and b"cells per axis" in lib.am_last_error()
    a.grid.cells, a.grid.n_points = 4, 0
    assert lib.am_nn_grid_build(C.byref(a), None) != 0 and b"empty" in lib.am_last_error()
    a.grid.n_points = 10
    assert lib.am_nn_grid_build(C.byref(a), None) != 0 and b"null grid pointer" in lib.am_last_error()
    for f in ("frame", "slabs", "cell_start", "order", "sorted"):
        setattr(a.grid, f, 4096)
    a.grid.sorted = 4100
    assert lib.am_nn_grid_build(C.byref(a), None) != 0 and b"16-byte aligned" in lib.am_last_error()
    a.grid.sorted, a.points = 4096, 4096
    a.workspace, a.workspace_bytes = 4096, lib.am_nn_grid_workspace_bytes(10, 1, 4) - 1
    assert lib.am_nn_grid_cells(C.byref(a), None) != 0 and b"workspace" in lib.am_last_error()
    s = L.AmNnGridSearchArgs()
    s.grid = a.grid
    s.batch, s.n_queries = 1, 0
    assert lib.am_nn_grid_search(C.byref(s), None) != 0 and b"empty" in lib.am_last_error()
    s.n_queries, s.batch, s.grid.batch = 5, 3, 2
    assert lib.am_nn_grid_search(C.byref(s), None) != 0 and b"one shared grid or one each" in lib.am_last_error()
    s.grid.batch = 1
    assert lib.am_nn_grid_search(C.byref(s), None) != 0 and b"null pointer" in lib.am_last_error()
    for fn in (ops.nn_grid_build, lambda t: ops.nearest_neighbors_grid(t, t)):          # no CPU path
        with pytest.raises(RuntimeError):
            fn(torch.zeros(4, 3))
    with pytest.raises(ValueError):
        ops.NnGrid(10, 1, 129, True, "cpu")
