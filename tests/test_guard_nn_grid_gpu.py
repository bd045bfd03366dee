"""Guard bands and exact buffers of the grid nearest-neighbour search - am_nn_grid_cells, am_nn_grid_build, am_nn_grid_search - called
through the C ABI itself.  Every output lies in an arena of sentinels (tests/_guard.py), every input in a poisoned one, the grid in a
uint8 arena of EXACTLY am_nn_grid_bytes and the workspace in one of exactly am_nn_grid_workspace_bytes, once left at the sentinel and
once zeroed.  A workspace one byte short is refused on the host and nothing is launched; a grid whose cell_start is not ascending or
passes the points, and an `order` entry outside the points, raise the flag word and write nothing outside the outputs."""
import ctypes as C

import numpy as np
import pytest
import torch

import _nn_grid_ref as R
from _guard import SENTINEL, Arena, Padded64
from actionmesh_amd import _lib as L
from actionmesh_amd import ops

pytestmark = pytest.mark.gpu
OUT64 = -7.25e300


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return L.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Input:
    def __init__(self, t, dev):
        self.a = Arena.flat_of(t.contiguous().to(dev))
        self.ptr = self.a.view.data_ptr()
        self.before = self.a.bits.clone()

    def unchanged(self, what):
        assert torch.equal(self.a.bits, self.before), f"{what}: the input or its guards changed"


class Problem:
    """One (P, Q, B, G) problem with every buffer in an arena; cells() / build() / search() call the C ABI and check the guards."""

    def __init__(self, dev, lib, P, Q, B, G, zero=False):
        self.dev, self.lib, self.P, self.Q, self.B, self.G = dev, lib, P, Q, B, G
        g = torch.Generator().manual_seed(P + Q + G)
        self.pts, self.qry = torch.randn((B, P, 3), generator=g), torch.randn((B, Q, 3), generator=g)
        self.pts[:, P - 1] = self.pts[:, 1]              # a duplicate in the last row: the lower index wins
        self.qry[:, Q - 1] = self.pts[:, 1]
        self.PA, self.QA = Input(self.pts, dev), Input(self.qry, dev)
        self.need_grid, self.need_ws = lib.am_nn_grid_bytes(P, B, G), lib.am_nn_grid_workspace_bytes(P, B, G)
        assert self.need_grid == sum((n + 15) // 16 * 16 for n in (B * 32, B * 24 * G, B * (G ** 3 + 2) * 4, B * P * 4, B * P * 16))
        assert self.need_ws == (B * (8 + 6 * G) * 4 + 15) // 16 * 16 + (B * P * 4 + 15) // 16 * 16
        self.GA = Arena.flat((self.need_grid,), torch.uint8, dev)
        self.WA = Arena.flat((self.need_ws,), torch.uint8, dev)
        if zero:
            self.WA.view.zero_(), self.GA.view.zero_()
        self.grid = ops.NnGrid(P, B, G, False, dev, buffer=self.GA.view)
        self.cell = Arena.flat((B, P), torch.int32, dev)
        self.flag = Arena.flat((1,), torch.int32, dev)

    def build_args(self, ws_bytes=None):
        a = L.AmNnGridBuildArgs()
        a.points, a.points_bstride, a.grid = self.PA.ptr, self.P * 3, self.grid.struct()
        a.out_cell, a.out_flag = self.cell.view.data_ptr(), self.flag.view.data_ptr()
        a.workspace, a.workspace_bytes = self.WA.view.data_ptr(), self.need_ws if ws_bytes is None else ws_bytes
        return a

    def guards(self):
        torch.cuda.synchronize()
        for name, a in (("grid", self.GA), ("workspace", self.WA), ("out_cell", self.cell), ("out_flag", self.flag)):
            a.assert_untouched(name)
        self.PA.unchanged("points"), self.QA.unchanged("queries")

    def cells(self):
        a = self.build_args()
        assert self.lib.am_nn_grid_cells(C.byref(a), stream()) == 0, self.lib.am_last_error()
        self.guards()

    def sort(self):
        self.grid.order.copy_(torch.sort(self.cell.view, dim=1, stable=True).indices)

    def build(self):
        a = self.build_args()
        assert self.lib.am_nn_grid_build(C.byref(a), stream()) == 0, self.lib.am_last_error()
        self.guards()
        return int(self.flag.view[0])

    def search(self, precise, query_order=None):
        idx = Arena.flat((self.B, self.Q), torch.int32, self.dev)
        d2 = Padded64((self.B, self.Q), self.dev, OUT64) if precise else Arena.flat((self.B, self.Q), torch.float32, self.dev)
        a = L.AmNnGridSearchArgs()
        a.grid, a.queries, a.n_queries, a.queries_bstride = self.grid.struct(), self.QA.ptr, self.Q, self.Q * 3
        a.batch, a.precise = self.B, precise
        if query_order is not None:
            a.query_order, a.query_order_bstride = query_order.ptr, self.Q
        a.out_index, a.out_d2, a.out_flag = idx.view.data_ptr(), d2.view.data_ptr(), self.flag.view.data_ptr()
        before = self.GA.bits.clone()
        assert self.lib.am_nn_grid_search(C.byref(a), stream()) == 0, self.lib.am_last_error()
        self.guards()
        idx.assert_untouched("out_index")
        d2.assert_untouched("out_d2", written=True) if precise else d2.assert_untouched("out_d2")
        assert torch.equal(self.GA.bits, before), "the search wrote the grid"
        if query_order is not None:
            query_order.unchanged("query_order")
        return idx.view.clone(), d2.view.clone(), int(self.flag.view[0])


@pytest.mark.parametrize("P,Q,B,G", [(513, 7, 1, 9), (2049, 257, 3, 16), (5, 1025, 2, 3)])
def test_guards_and_exact_buffers(dev, lib, P, Q, B, G):
    results = []
    for zero in (False, True):
        pr = Problem(dev, lib, P, Q, B, G, zero)
        pr.cells(), pr.sort()
        assert pr.build() == 0
        qo = Input(ops.nn_grid_build(pr.qry.to(dev), cells=G).order, dev)
        out = {}
        for precise in (0, 1):
            idx, d2, flag = pr.search(precise)
            assert flag == 0
            for b in range(B):
                ri, rd = R.brute(pr.pts[b].numpy(), pr.qry[b].numpy(), np.float64 if precise else np.float32)
                assert np.array_equal(idx[b].cpu().numpy(), ri)
                assert np.array_equal(d2[b].cpu().numpy().view(np.uint8), rd.view(np.uint8))
            assert (idx[:, Q - 1] == 1).all()
            idx2, d22, flag = pr.search(precise, qo)
            assert flag == 0 and torch.equal(idx2, idx) and torch.equal(d22.view(torch.uint8), d2.view(torch.uint8))
            out[precise] = (idx, d2)
        g = pr.grid
        results.append(([t.clone().view(torch.uint8) for t in (g.frame, g.slabs, g.cell_start, g.order, g.sorted)], out))
    # neither the grid's arrays (the padding between them is nobody's) nor the results depend on what the buffers held
    assert all(torch.equal(a, b) for a, b in zip(results[0][0], results[1][0])), "the grid depends on what the buffers held"
    for precise in (0, 1):
        assert torch.equal(results[0][1][precise][0], results[1][1][precise][0])


def test_workspace_one_byte_short_launches_nothing(dev, lib):
    pr = Problem(dev, lib, 700, 50, 2, 8)
    for fn in (lib.am_nn_grid_cells, lib.am_nn_grid_build):
        a = pr.build_args(pr.need_ws - 1)
        assert fn(C.byref(a), stream()) != 0
        msg = lib.am_last_error().decode()
        assert "workspace" in msg and str(pr.need_ws) in msg, msg
    pr.guards()
    assert (pr.cell.view == SENTINEL[torch.int32]).all() and (pr.GA.view == 0xA5).all() and (pr.WA.view == 0xA5).all(), "something was launched"
    assert int(pr.flag.view[0]) == SENTINEL[torch.int32]


def _built(dev, lib):
    pr = Problem(dev, lib, 700, 300, 2, 8)
    pr.cells(), pr.sort()
    assert pr.build() == 0
    return pr


@pytest.mark.parametrize("case", ["not_monotone", "past_the_points"])
def test_bad_cell_start_is_reported_and_writes_nothing_outside(dev, lib, case):
    pr = _built(dev, lib)
    if case == "not_monotone":
        pr.grid.cell_start.copy_(pr.grid.cell_start.flip(1))            # descending: begin > end wherever points lie
    else:
        pr.grid.cell_start.add_(pr.P + 1)                               # every range lies past the sorted copy
    for precise in (0, 1):
        idx, d2, flag = pr.search(precise)                              # the guards are checked inside
        assert flag & L.NN_GRID_BAD_CELL_START
        assert (idx == -1).all() and torch.isinf(d2).all()              # "no neighbour": nothing was read through a bad range
    grid = pr.grid
    with pytest.raises(ValueError, match="cell_start"):
        ops.nn_grid_search(grid, pr.qry.to(dev))
    ops.nn_grid_search(grid, pr.qry.to(dev), check=False)
    with pytest.raises(ValueError, match="cell_start"):
        ops.nn_grid_valid([grid])


@pytest.mark.parametrize("value", [700, 2 ** 31 - 1, -1, -2 ** 31], ids=["P", "int32_max", "minus_one", "int32_min"])
def test_bad_order_entry_is_reported_and_writes_nothing_outside(dev, lib, value):
    pr = Problem(dev, lib, 700, 300, 2, 8)
    pr.cells(), pr.sort()
    good = int(pr.grid.order[1, 13])
    pr.grid.order[1, 13] = value
    assert pr.build() & L.NN_GRID_BAD_ORDER                             # the guards are checked inside
    rec = pr.grid.sorted[1, 13].cpu()
    assert torch.isnan(rec[:3]).all() and int(rec[3:].view(torch.int32)) == -1
    for precise in (0, 1):                                              # whatever such a grid holds, searching it stays inside the buffers
        idx, d2, flag = pr.search(precise)
        assert (idx[1] != good).all() and (idx[0] >= 0).all()


def test_bad_sorted_index_is_reported(dev, lib):
    pr = _built(dev, lib)
    pr.grid.sorted[0].view(torch.int32)[:, 3] = pr.P
    idx, d2, flag = pr.search(0)
    assert flag & L.NN_GRID_BAD_INDEX and (idx[0] == -1).all() and (idx[1] >= 0).all()
