"""The grid nearest-neighbour search on the device: the build's arrays against the numpy restatement bit for bit, and the search
against am_nn_search (ops.nearest_neighbors, the brute-force kernel): the same index and the same d2 bits on every query, in both
precisions - the CPU file's edge cases plus shapes that cross a workgroup, the grid stride and the batch."""
import os

import numpy as np
import pytest
import torch

import _nn_grid_ref as R
from actionmesh_amd import ops
from test_nn_grid_cpu import CASES, RUNS

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "actionbench.npz")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().cpu().numpy().view(np.uint8)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def assert_equals_brute(points, queries, **grid_args):
    for precise in (False, True):
        bi, bd = ops.nearest_neighbors(points, queries, precise=precise, check=False)
        grid = ops.nn_grid_build(points, **grid_args)
        gi, gd = ops.nn_grid_search(grid, queries, precise=precise, check=False)
        ops.nn_grid_valid([grid])
        assert same(gi, bi), (precise, (gi != bi).nonzero()[:8])
        assert same(gd, bd), precise
    return gi, gd


@pytest.mark.parametrize("name,G", RUNS, ids=[f"{n}-G{g or 'default'}" for n, g in RUNS])
def test_build_equals_the_restatement_and_search_equals_brute_force(dev, name, G):
    pts, qry, _ = CASES[name]
    ref = R.build(pts, R.default_cells(len(pts)) if G is None else G)
    tp, tq = torch.from_numpy(pts).to(dev), torch.from_numpy(qry).to(dev)
    grid = ops.nn_grid_build(tp, cells=G)
    assert grid.cells == ref["cells"] and grid.shared and grid.batch == 1
    assert np.array_equal(bits(grid.frame[0]), ref["frame"].view(np.uint8)), (grid.frame.cpu().numpy(), ref["frame"])
    assert np.array_equal(grid.order[0].cpu().numpy(), ref["order"])
    assert np.array_equal(grid.cell_start[0].cpu().numpy(), ref["cell_start"])
    assert np.array_equal(bits(grid.sorted[0]), ref["sorted"].view(np.uint8))
    assert np.array_equal(bits(grid.slabs[0]), ref["slabs"].view(np.uint8)), (grid.slabs.cpu().numpy(), ref["slabs"])
    assert_equals_brute(tp, tq, cells=G)


@pytest.mark.parametrize("P,Q,B,shared", [(513, 7, 1, False), (5000, 3000, 1, False), (2049, 1025, 3, False), (2000, 2000, 24, False),
                                          (2000, 2000, 24, True)])
def test_shapes_and_batches_equal_brute_force(dev, P, Q, B, shared):
    g = torch.Generator().manual_seed(P * 31 + Q + B)
    u = torch.randn((B, P, 3), generator=g)
    pts = u / u.norm(dim=-1, keepdim=True) * torch.tensor([1.0, 0.7, 0.4])           # an ellipsoid's surface, like the metric's clouds
    pts[:, P // 2] = pts[:, 3]                                                       # a duplicate: index 3 wins
    qry = pts[:, torch.randperm(P, generator=g)[:Q] % P] + 0.01 * torch.randn((B, Q, 3), generator=g)
    if shared:
        pts[1:] = pts[:1]                                                            # the batch searches entry 0's cloud
    qry[:, 0] = pts[:, 3]
    qry[:, Q - 1] = torch.tensor([9.0, -9.0, 9.0])                                   # far outside the box
    tp, tq = (pts[0] if shared else pts).contiguous().to(dev), qry.contiguous().to(dev)
    gi, gd = assert_equals_brute(tp, tq)
    assert gi.shape == (B, Q) and (gi[:, 0] == 3).all() and (gd[:, 0] == 0).all()
    if B == 1:                       # 2-D operands: 1-D results, like nearest_neighbors
        i1, d1 = ops.nearest_neighbors_grid(tp[0], tq[0])
        assert i1.shape == (Q,) and same(i1, gi[0]) and same(d1, gd[0])


def test_query_order_changes_nothing_and_runs_repeat(dev):
    g = torch.Generator().manual_seed(11)
    pts, qry = torch.randn((3, 1500, 3), generator=g).to(dev), torch.randn((3, 1100, 3), generator=g).to(dev)
    grid = ops.nn_grid_build(pts)
    base = ops.nn_grid_search(grid, qry, precise=False)
    own = ops.nn_grid_build(qry).order                                               # the query clouds' own cell order, per entry
    perm = torch.randperm(1100, generator=g).to(torch.int32).to(dev)                 # one permutation shared by the batch
    for qo in (own, perm, perm[None].contiguous()):
        got = ops.nn_grid_search(grid, qry, precise=False, query_order=qo)
        assert same(got[0], base[0]) and same(got[1], base[1])
    again = ops.nn_grid_search(ops.nn_grid_build(pts), qry, precise=False)           # a second build and run: identical
    assert same(again[0], base[0]) and same(again[1], base[1])
    bad = perm.clone()
    bad[5] = 1100
    with pytest.raises(ValueError, match="query_order"):
        ops.nn_grid_search(grid, qry, precise=False, query_order=bad)
    ops.nn_grid_search(grid, qry, precise=False, query_order=bad, check=False)
    with pytest.raises(ValueError, match="query_order"):
        ops.nn_grid_valid([grid])
    ops.nn_grid_valid([grid])                                                        # the deferred flag is consumed


def test_gold_fixture_neighbours_bit_for_bit(dev):
    gold = np.load(GOLD)
    p, g = torch.from_numpy(gold["preds"][0]).to(dev), torch.from_numpy(gold["gts"][0]).to(dev)
    idx, d2 = ops.nearest_neighbors_grid(p, g)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float64
    assert np.array_equal(idx.cpu().numpy(), gold["nn_idx_gt_to_pred"]) and np.array_equal(np.sqrt(d2.cpu().numpy()), gold["nn_dist_gt_to_pred"])
    idx, d2 = ops.nearest_neighbors_grid(g, p)
    assert np.array_equal(idx.cpu().numpy(), gold["nn_idx_pred_to_gt"]) and np.array_equal(np.sqrt(d2.cpu().numpy()), gold["nn_dist_pred_to_gt"])


def test_errors_are_nearest_neighbors_errors(dev):
    with pytest.raises(ValueError):
        ops.nearest_neighbors_grid(torch.zeros((0, 3), device=dev), torch.zeros((2, 3), device=dev))
    with pytest.raises(ValueError):
        ops.nearest_neighbors_grid(torch.zeros((4, 2), device=dev), torch.zeros((2, 3), device=dev))
    with pytest.raises(ValueError):
        ops.nearest_neighbors_grid(torch.zeros((2, 4, 3), device=dev), torch.zeros((3, 2, 3), device=dev))
    with pytest.raises(TypeError):
        ops.nearest_neighbors_grid(torch.zeros((4, 3), device=dev, dtype=torch.float64), torch.zeros((2, 3), device=dev))
    with pytest.raises(ValueError, match="no finite distance"):
        ops.nearest_neighbors_grid(torch.zeros((4, 3), device=dev), torch.full((2, 3), float("nan"), device=dev))
    with pytest.raises(ValueError):
        ops.nn_grid_build(torch.zeros((4, 3), device=dev), cells=129)
