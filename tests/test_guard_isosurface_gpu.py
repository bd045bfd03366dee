"""The three iso-surface kernels (csrc/am_isosurface.hip) one by one against the numpy restatement of the header
(tests/_isosurface_ref.py), bit for bit, with every output in a sentinel-padded buffer and every input in a poisoned one (NaN around
the values, a mask above 127 and offsets far outside the mesh around the tables), as tests/test_mesh_decimate_gpu.py does - and the
flag on corrupted tables: the kernels compare every offset with its bound themselves, so nothing outside the outputs is written."""
import numpy as np
import pytest
import torch

import _isosurface_ref as R

pytestmark = pytest.mark.gpu

PAD = 1024                      # elements in front of and behind a padded buffer
FILL = {torch.float32: float("nan"), torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A, torch.uint8: 0xA5}
OUT_FILL = {torch.float32: -7.25e30, torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A, torch.uint8: 0xA5}
BITS = {torch.float32: torch.int32, torch.int32: torch.int32, torch.int64: torch.int64, torch.uint8: torch.uint8}
GRIDS = {"sphere17": lambda: (R.sphere(17),) + R.frame(17), "torus17": lambda: (R.torus(17),) + R.frame(17),
         "noncubic": R.noncubic_with_nans}
_tables = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from actionmesh_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


class Padded:
    """A contiguous tensor with PAD sentinels on each side: an input (`data`: a numpy array; poisoned guards) or an output (`shape`)."""

    def __init__(self, dev, data=None, shape=None, dtype=None):
        if data is not None:
            data = torch.from_numpy(np.ascontiguousarray(data))
            shape, dtype, fill = tuple(data.shape), data.dtype, FILL[data.dtype]
        else:
            fill = OUT_FILL[dtype]
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=dev)
        self.view = self.buf[PAD:PAD + n].view(shape)
        if data is not None:
            self.view.copy_(data)
        self.before, self.n, self.bits = self.buf.clone(), n, BITS[dtype]

    def check(self, what, written=False):
        now, was = self.buf.view(self.bits), self.before.view(self.bits)
        assert torch.equal(now[:PAD], was[:PAD]) and torch.equal(now[PAD + self.n:], was[PAD + self.n:]), f"{what}: a guard changed"
        if not written:
            assert torch.equal(now, was), f"{what}: an input changed"


def same_bits(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def tables(name):
    """The restatement's tables and results for one grid, once; copies, so a test may corrupt its own."""
    if name not in _tables:
        values, origin, spacing = GRIDS[name]()
        s = dict(values=values, origin=origin, spacing=spacing)
        s["mask"], s["count"] = R.ref_classify(values)
        s["voff"], s["toff"], s["V"], s["F"] = R.offsets_of(s["mask"], s["count"])
        s["vertices"] = R.ref_vertices(values, s["mask"], s["voff"], s["V"], origin, spacing)
        s["faces"] = R.ref_triangles(values, s["mask"], s["count"], s["voff"], s["toff"], s["V"], s["F"])
        _tables[name] = s
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _tables[name].items()}


@pytest.mark.parametrize("name", list(GRIDS))
def test_each_kernel_bit_identical_inside_guards(dev, name):
    from actionmesh_amd import ops
    s = tables(name)
    shape, V, F = s["values"].shape, s["V"], s["F"]
    assert V > 500 and F > 1000
    inp = {k: Padded(dev, data=s[k]) for k in ("values", "mask", "count", "voff", "toff")}

    def inputs_untouched():
        for k, p in inp.items():
            p.check(k)

    mask, count = Padded(dev, shape=shape, dtype=torch.uint8), Padded(dev, shape=shape, dtype=torch.uint8)
    got = ops.iso_classify(inp["values"].view, 0.0, True, out_mask=mask.view, out_count=count.view)
    torch.cuda.synchronize()
    assert got[0] is mask.view and got[1] is count.view
    mask.check("mask", written=True)
    count.check("count", written=True)
    inputs_untouched()
    assert same_bits(mask.view, s["mask"]) and same_bits(count.view, s["count"])
    # the other comparison on the negated values: the same tables
    negated = Padded(dev, data=-s["values"])
    other = ops.iso_classify(negated.view, 0.0, False)
    assert same_bits(other[0], s["mask"]) and same_bits(other[1], s["count"])

    vertices = Padded(dev, shape=(V, 3), dtype=torch.float32)
    assert ops.iso_vertices(inp["values"].view, inp["mask"].view, inp["voff"].view, V, s["origin"], s["spacing"], 0.0, out=vertices.view) is vertices.view
    torch.cuda.synchronize()
    vertices.check("vertices", written=True)
    inputs_untouched()
    assert same_bits(vertices.view, s["vertices"])

    faces = Padded(dev, shape=(F, 3), dtype=torch.int32)
    assert ops.iso_triangles(inp["values"].view, inp["mask"].view, inp["count"].view, inp["voff"].view, inp["toff"].view, V, F, 0.0, True,
                             out=faces.view) is faces.view
    torch.cuda.synchronize()
    faces.check("faces", written=True)
    inputs_untouched()
    assert same_bits(faces.view, s["faces"])


def test_a_level_other_than_zero(dev):
    from actionmesh_amd import ops
    values, origin, spacing = R.noncubic_with_nans()
    mask, count = R.ref_classify(values, 0.25)
    voff, toff, V, F = R.offsets_of(mask, count)
    t = torch.from_numpy(values).to(dev)
    got_mask, got_count = ops.iso_classify(t, 0.25)
    assert same_bits(got_mask, mask) and same_bits(got_count, count)
    tv, tt = torch.from_numpy(voff).to(dev), torch.from_numpy(toff).to(dev)
    assert same_bits(ops.iso_vertices(t, got_mask, tv, V, origin, spacing, 0.25), R.ref_vertices(values, mask, voff, V, origin, spacing, 0.25))
    assert same_bits(ops.iso_triangles(t, got_mask, got_count, tv, tt, V, F, 0.25), R.ref_triangles(values, mask, count, voff, toff, V, F, 0.25))


CORRUPTIONS = ["vertex offset past V", "vertex offset negative", "vertex offset huge", "triangle offset past F", "triangle offset negative",
               "mask for an edge that leaves the grid", "mask above 127", "count where no cell starts", "count too large",
               "count too small"]


@pytest.mark.parametrize("what", CORRUPTIONS)
def test_corrupted_tables_raise_through_the_flag(dev, what):
    """No offset is used as an address before it is compared with its bound: the call returns, nothing outside the outputs is
    written, and the flag raises."""
    from actionmesh_amd import ops
    s = tables("sphere17")
    shape, V, F = s["values"].shape, s["V"], s["F"]
    crossing = np.argwhere((s["mask"] != 0) & (s["count"] != 0))[40]           # a point that starts edges and a cell with triangles
    cell = tuple(np.argwhere(s["count"] >= 2)[100])                            # not the last one: its rows are followed by others
    at = tuple(crossing)
    raising = ("vertices", "triangles")
    if what == "vertex offset past V":
        s["voff"][at] = V + 5
    elif what == "vertex offset negative":
        s["voff"][at] = -3
    elif what == "vertex offset huge":
        s["voff"][at] = 2 ** 63 - 2
    elif what == "triangle offset past F":
        s["toff"][cell], raising = F - int(s["count"][cell]) + 1, ("triangles",)
    elif what == "triangle offset negative":
        s["toff"][cell], raising = -1, ("triangles",)
    elif what == "mask for an edge that leaves the grid":
        s["mask"][8, 8, shape[2] - 1], raising = 1, ("vertices",)
    elif what == "mask above 127":
        s["mask"][at] |= 128
    elif what == "count where no cell starts":
        s["count"][shape[0] - 1, 3, 3], raising = 2, ("triangles",)
    elif what == "count too large":
        s["count"][cell], raising = s["count"][cell] + 1, ("triangles",)
    elif what == "count too small":
        s["count"][cell], raising = s["count"][cell] - 1, ("triangles",)
    inp = {k: Padded(dev, data=s[k]) for k in ("values", "mask", "count", "voff", "toff")}
    outs = {"vertices": Padded(dev, shape=(V, 3), dtype=torch.float32), "triangles": Padded(dev, shape=(F, 3), dtype=torch.int32)}
    calls = {
        "vertices": lambda: ops.iso_vertices(inp["values"].view, inp["mask"].view, inp["voff"].view, V, s["origin"], s["spacing"], 0.0,
                                             out=outs["vertices"].view),
        "triangles": lambda: ops.iso_triangles(inp["values"].view, inp["mask"].view, inp["count"].view, inp["voff"].view, inp["toff"].view,
                                               V, F, 0.0, True, out=outs["triangles"].view),
    }
    for name in raising:
        with pytest.raises(ValueError, match="iso_" + name):
            calls[name]()
    torch.cuda.synchronize()
    for name, p in outs.items():
        p.check(name, written=True)
    for k, p in inp.items():
        p.check(k)


def test_bad_arguments_are_refused_before_any_launch(dev):
    from actionmesh_amd import ops
    t = torch.zeros((3, 3, 3), device=dev)
    with pytest.raises(ValueError, match="at least 2"):
        ops.iso_classify(torch.zeros((1, 3, 3), device=dev))
    with pytest.raises(ValueError, match="finite"):
        ops.iso_classify(t, float("inf"))
    with pytest.raises(ValueError, match="mask"):
        ops.iso_vertices(t, torch.zeros((3, 3, 2), dtype=torch.uint8, device=dev), torch.zeros((3, 3, 3), dtype=torch.int64, device=dev), 1,
                         (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match="outside 1"):
        ops.iso_triangles(t, *(torch.zeros((3, 3, 3), dtype=d, device=dev) for d in (torch.uint8, torch.uint8, torch.int64, torch.int64)), 0, 1)
