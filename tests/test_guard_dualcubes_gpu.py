"""The four dual-marching-cubes kernels (csrc/am_dualcubes.hip) one by one against the numpy restatement of the header
(tests/_dualcubes_ref.py), bit for bit, with every output inside a guard band and every input in a poisoned arena (tests/_guard.py:
NaN around the values, codes above 511, masks above 7 and offsets far outside the mesh around the tables) - and the flag on corrupted
tables: the kernels compare every offset, code and index with its bound themselves, so nothing outside the outputs is written."""
import numpy as np
import pytest
import torch

import _dualcubes_ref as D
import _isosurface_ref as R
from _guard import Arena

pytestmark = pytest.mark.gpu

_tables = {}
# the arena dtype that carries a dtype _guard.py has no sentinel for, and how many of its elements make one
CARRIER = {torch.int16: (torch.uint8, 2), torch.int64: (torch.int32, 2)}


def tunnel():
    values = np.ones((4, 4, 4), dtype=np.float32)
    values[1, 2, 2] = values[2, 1, 2] = -1.0
    return values, (0.0,) * 3, (1.0,) * 3


def noise():
    values = np.random.default_rng(0).standard_normal((21, 21, 21))
    for s in (0, -1):
        values[s], values[:, s], values[:, :, s] = -1.0, -1.0, -1.0
    return values.astype(np.float32), (-1.0, 0.5, 2.0), (0.1, 0.1, 0.1)


def across_tiles():
    """21 x 13 x 70 points: more than one am_dmc_cells tile along every axis (8 x 8 x 64 points each), none of them full."""
    i, j, k = np.meshgrid(np.arange(21), np.arange(13), np.arange(70), indexing="ij")
    values = (np.sin(0.45 * i + 0.2) * np.cos(0.6 * j) + np.sin(0.31 * k - 0.4) * 0.8 - 0.1).astype(np.float32)
    values[7, 8, 63], values[8, 7, 64] = np.nan, np.nan            # next to the tile corners
    return values, (1.0, -2.0, 0.5), (0.5, 1.25, 0.75)


GRIDS = {"sphere17": lambda: (R.sphere(17),) + R.frame(17), "torus17": lambda: (R.torus(17),) + R.frame(17),
         "noncubic": R.noncubic_with_nans, "tunnel": tunnel, "noise21": noise, "across_tiles": across_tiles}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from actionmesh_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


class Guarded:
    """A contiguous tensor inside a tests/_guard.py arena: an input (`data`: a numpy array; the guards poison what reads them) or an
    output (`shape`, `dtype`)."""

    def __init__(self, dev, data=None, shape=None, dtype=None):
        if data is not None:
            data = torch.from_numpy(np.ascontiguousarray(data))
            shape, dtype = tuple(data.shape), data.dtype
        carrier, per = CARRIER.get(dtype, (dtype, 1))
        self.arena = Arena.flat(tuple(shape[:-1]) + (shape[-1] * per,), carrier, dev)
        self.view = self.arena.view.view(dtype)
        assert tuple(self.view.shape) == tuple(shape) and self.view.is_contiguous()
        if data is not None:
            self.view.copy_(data)
        self.before = self.view.clone()

    def check(self, what, written=False):
        self.arena.assert_untouched(what)
        if not written:
            assert torch.equal(self.view.view(torch.uint8), self.before.view(torch.uint8)), f"{what}: an input changed"


def same_bits(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def tables(name):
    """The restatement's tables and results for one grid, once; copies, so a test may corrupt its own."""
    if name not in _tables:
        values, origin, spacing = GRIDS[name]()
        s = D.ref_tables(values, 0.0, origin, spacing)
        s.update(values=values, origin=origin, spacing=spacing)
        _tables[name] = s
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _tables[name].items()}


INPUTS = ("values", "config", "double", "code", "emask", "voff", "toff", "vertices")


@pytest.mark.parametrize("name", list(GRIDS))
def test_each_kernel_bit_identical_inside_guards(dev, name):
    from actionmesh_amd import ops
    s = tables(name)
    shape, V, F = s["values"].shape, s["V"], s["F"]
    assert V >= 16 and F >= 24
    if name in ("tunnel", "noise21"):
        assert (s["code"] >> 8).any()                              # flipped faces
    inp = {k: Guarded(dev, data=s[k]) for k in INPUTS}

    def inputs_untouched():
        for k, g in inp.items():
            g.check(k)

    config, double = (Guarded(dev, shape=shape, dtype=torch.uint8) for _ in range(2))
    got = ops.dmc_cells(inp["values"].view, 0.0, True, out_config=config.view, out_double=double.view)
    torch.cuda.synchronize()
    assert got[0] is config.view and got[1] is double.view
    config.check("config", written=True)
    double.check("double", written=True)
    inputs_untouched()
    assert same_bits(config.view, s["config"]) and same_bits(double.view, s["double"])
    # the other comparison on the negated values: the same tables
    other = ops.dmc_cells(Guarded(dev, data=-s["values"]).view, 0.0, False)
    assert same_bits(other[0], s["config"]) and same_bits(other[1], s["double"])

    code = Guarded(dev, shape=shape, dtype=torch.int16)
    count, emask = (Guarded(dev, shape=shape, dtype=torch.uint8) for _ in range(2))
    got = ops.dmc_classify(inp["config"].view, inp["double"].view, out_code=code.view, out_count=count.view, out_edge_mask=emask.view)
    torch.cuda.synchronize()
    assert got[0] is code.view and got[1] is count.view and got[2] is emask.view
    for what, g in (("code", code), ("count", count), ("emask", emask)):
        g.check(what, written=True)
        assert same_bits(g.view, s[what]), what
    inputs_untouched()

    vertices = Guarded(dev, shape=(V, 3), dtype=torch.float32)
    assert ops.dmc_vertices(inp["values"].view, inp["code"].view, inp["voff"].view, V, s["origin"], s["spacing"], 0.0, True,
                            out=vertices.view) is vertices.view
    torch.cuda.synchronize()
    vertices.check("vertices", written=True)
    inputs_untouched()
    assert same_bits(vertices.view, s["vertices"])

    faces = Guarded(dev, shape=(F, 3), dtype=torch.int32)
    assert ops.dmc_triangles(inp["code"].view, inp["emask"].view, inp["voff"].view, inp["toff"].view, inp["vertices"].view, V, F,
                             out=faces.view) is faces.view
    torch.cuda.synchronize()
    faces.check("faces", written=True)
    inputs_untouched()
    assert same_bits(faces.view, s["faces"])


def test_a_level_other_than_zero(dev):
    from actionmesh_amd import ops
    values, origin, spacing = R.noncubic_with_nans()
    s = D.ref_tables(values, 0.25, origin, spacing)
    t = torch.from_numpy(values).to(dev)
    config, double = ops.dmc_cells(t, 0.25)
    code, count, emask = ops.dmc_classify(config, double)
    assert same_bits(config, s["config"]) and same_bits(code, s["code"]) and same_bits(count, s["count"]) and same_bits(emask, s["emask"])
    tv, tt = torch.from_numpy(s["voff"]).to(dev), torch.from_numpy(s["toff"]).to(dev)
    vertices = ops.dmc_vertices(t, code, tv, s["V"], origin, spacing, 0.25)
    assert same_bits(vertices, s["vertices"])
    assert same_bits(ops.dmc_triangles(code, emask, tv, tt, vertices, s["V"], s["F"]), s["faces"])


CORRUPTIONS = ["vertex offset negative", "vertex offset past V", "vertex offset huge", "triangle offset negative",
               "triangle offset past F", "code above 511", "code with the configuration 255", "code of another configuration",
               "flip bit on a cell without a double face", "code where no cell starts", "edge mask on the grid's last plane",
               "edge mask above 7", "edge mask next to an inactive cell"]


@pytest.mark.parametrize("what", CORRUPTIONS)
def test_corrupted_tables_raise_through_the_flag(dev, what):
    """Ordinary bounds checks on host-supplied tables: no offset, code or index is used as an address before it is compared with
    its bound, so the call returns, nothing outside the outputs is written, and the flag raises."""
    from actionmesh_amd import ops
    s = tables("sphere17")
    shape, V, F = s["values"].shape, s["V"], s["F"]
    at = tuple(np.argwhere(s["emask"] != 0)[40])                   # an active cell, one of the four around an emitting edge
    assert s["code"][at] != 0 and D.DOUBLE[s["code"][at] & 255] == 0
    raising = ("vertices", "triangles")
    if what == "vertex offset negative":
        s["voff"][at] = -3
    elif what == "vertex offset past V":
        s["voff"][at] = V
    elif what == "vertex offset huge":
        s["voff"][at] = 2 ** 63 - 2
    elif what == "triangle offset negative":
        s["toff"][at], raising = -1, ("triangles",)
    elif what == "triangle offset past F":
        s["toff"][at], raising = F - 2 * int(R.POPCOUNT[s["emask"][at]]) + 1, ("triangles",)
    elif what == "code above 511":
        s["code"][at] += 512
    elif what == "code with the configuration 255":
        s["code"][at] = 255
    elif what == "code of another configuration":
        s["code"][at], raising = s["code"][at] ^ 0x80, ("vertices",)       # corner 111 on the other side
        assert s["code"][at] not in (0, 255)
    elif what == "flip bit on a cell without a double face":
        s["code"][at] |= 256
    elif what == "code where no cell starts":
        s["code"][shape[0] - 1, 3, 3], raising = 1, ("vertices",)
    elif what == "edge mask on the grid's last plane":
        s["emask"][8, 8, shape[2] - 1], raising = 1, ("triangles",)
    elif what == "edge mask above 7":
        s["emask"][at], raising = s["emask"][at] | 8, ("triangles",)
    elif what == "edge mask next to an inactive cell":
        s["emask"][8, 8, 8], raising = 7, ("triangles",)
        assert s["code"][8, 8, 8] == 0
    inp = {k: Guarded(dev, data=s[k]) for k in INPUTS}
    outs = {"vertices": Guarded(dev, shape=(V, 3), dtype=torch.float32), "triangles": Guarded(dev, shape=(F, 3), dtype=torch.int32)}
    calls = {
        "vertices": lambda: ops.dmc_vertices(inp["values"].view, inp["code"].view, inp["voff"].view, V, s["origin"], s["spacing"], 0.0,
                                             True, out=outs["vertices"].view),
        "triangles": lambda: ops.dmc_triangles(inp["code"].view, inp["emask"].view, inp["voff"].view, inp["toff"].view,
                                               inp["vertices"].view, V, F, out=outs["triangles"].view),
    }
    for name in raising:
        with pytest.raises(ValueError, match="dmc_" + name):
            calls[name]()
    torch.cuda.synchronize()
    for name, g in outs.items():
        g.check(name, written=True)
    for k, g in inp.items():
        g.check(k)


def test_bad_arguments_are_refused_before_any_launch(dev):
    from actionmesh_amd import ops
    t = torch.zeros((3, 3, 3), device=dev)
    u8, i16, i64 = (lambda shape=(3, 3, 3), d=d: torch.zeros(shape, dtype=d, device=dev) for d in (torch.uint8, torch.int16, torch.int64))
    with pytest.raises(ValueError, match="at least 2"):
        ops.dmc_cells(torch.zeros((1, 3, 3), device=dev))
    with pytest.raises(ValueError, match="finite"):
        ops.dmc_cells(t, float("inf"))
    with pytest.raises(ValueError, match="double"):
        ops.dmc_classify(u8(), u8((3, 3, 2)))
    with pytest.raises(TypeError):
        ops.dmc_classify(i16(), u8())
    with pytest.raises(ValueError, match="code"):
        ops.dmc_vertices(t, i16((3, 3, 2)), i64(), 1, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match="outside 1"):
        ops.dmc_triangles(i16(), u8(), i64(), i64(), torch.zeros((1, 3), device=dev), 0, 1)
    with pytest.raises(ValueError, match="vertices"):
        ops.dmc_triangles(i16(), u8(), i64(), i64(), torch.zeros((2, 3), device=dev), 1, 2)
