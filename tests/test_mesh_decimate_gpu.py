"""Mesh decimation on the device (csrc/am_decimate.hip) against the numpy restatement of the header (tests/_decimate_ref.py), bit for
bit: each of the four kernels on the first-round state of two meshes - with every output in a sentinel-padded buffer and every input
in a poisoned one (NaN around the floats, an index far outside the mesh around the integers), as tests/test_guard_mesh_gpu.py does -
then the whole loop, the edge cases, the flag on corrupted tables, and process_mesh's keyword."""
import numpy as np
import pytest
import torch

import _decimate_ref as R

pytestmark = pytest.mark.gpu

PAD = 1024                      # elements in front of and behind a padded buffer
FILL = {torch.float64: float("nan"), torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A, torch.uint8: 0xA5}
OUT_FILL = {torch.float64: -7.25e300, torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A, torch.uint8: 0xA5}
BITS = {torch.float64: torch.int64, torch.int32: torch.int32, torch.int64: torch.int64, torch.uint8: torch.uint8}
MESHES = {"icosphere3": (lambda: R.icosphere(3), 200), "torus32x16": (lambda: R.torus(32, 16), 160),
          "jittered4": (lambda: R.jittered_icosphere(4), 512)}


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

    def numpy(self):
        return self.view.cpu().numpy()


class Topology:
    def __init__(self, offsets, corners):
        self.offsets, self.corners = offsets, corners


def same_bits(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def first_round(v, f):
    """The first round of the restatement: every table, every kernel's result."""
    V = v.shape[0]
    s = dict(V=V, pos=v.astype(np.float64), faces=f.astype(np.int32))
    s["offsets"], s["corners"] = R.np_topology(s["faces"], V)
    s["edges"], s["he2e"], s["count"] = R.np_edges(s["faces"], V)
    s["Q"] = R.ref_quadrics(s["pos"], s["faces"], s["offsets"], s["corners"])
    s["cand"], s["cost"], s["key"] = R.ref_edges(s["pos"], s["Q"], s["faces"], s["offsets"], s["corners"], s["edges"], s["he2e"], s["count"])
    s["m1"], s["m2"], s["sel"] = R.ref_select(V, s["edges"], s["key"])
    s["kept"] = np.nonzero(s["sel"])[0].astype(np.int32)[::-1].copy()           # any order
    s["pos2"], s["Q2"], s["faces2"], s["map2"] = s["pos"].copy(), s["Q"].copy(), s["faces"].copy(), np.arange(V, dtype=np.int32)
    s["dead"] = R.ref_apply(s["pos2"], s["Q2"], s["faces2"], s["offsets"], s["corners"], s["edges"], s["cand"], s["kept"], s["map2"])
    return s


@pytest.mark.parametrize("name", ["icosphere3", "torus32x16"])
def test_each_kernel_bit_identical_inside_guards(dev, name):
    from actionmesh_amd import ops
    s = first_round(*MESHES[name][0]())
    V, F, E = s["V"], s["faces"].shape[0], s["edges"].shape[0]
    assert s["sel"].sum() > 1 and (s["key"] != R.NO_KEY).sum() > s["sel"].sum()
    inp = {k: Padded(dev, data=s[k]) for k in ("pos", "faces", "offsets", "corners", "edges", "he2e", "count", "Q", "cand", "key", "kept")}
    topo = Topology(inp["offsets"].view, inp["corners"].view)

    def inputs_untouched():
        for k, p in inp.items():
            p.check(k)

    # quadrics
    q = Padded(dev, shape=(V, 10), dtype=torch.float64)
    assert ops.decimate_quadrics(inp["pos"].view, inp["faces"].view, topo, out=q.view) is q.view
    torch.cuda.synchronize()
    q.check("quadrics", written=True)
    inputs_untouched()
    assert same_bits(q.view, s["Q"])
    # edges
    cand, cost, key = (Padded(dev, shape=sh, dtype=dt) for sh, dt in (((E, 3), torch.float64), ((E,), torch.float64), ((E,), torch.int64)))
    ops.decimate_edges(inp["pos"].view, inp["Q"].view, inp["faces"].view, topo, inp["edges"].view, inp["he2e"].view, inp["count"].view,
                       out_positions=cand.view, out_cost=cost.view, out_key=key.view)
    torch.cuda.synchronize()
    for p, what in ((cand, "candidates"), (cost, "cost"), (key, "key")):
        p.check(what, written=True)
    inputs_untouched()
    assert same_bits(cand.view, s["cand"]) and same_bits(cost.view, s["cost"]) and same_bits(key.view, s["key"])
    # select
    m1, m2, sel = (Padded(dev, shape=sh, dtype=dt) for sh, dt in (((V,), torch.int64), ((V,), torch.int64), ((E,), torch.uint8)))
    ops.decimate_select(V, inp["faces"].view, topo, inp["edges"].view, inp["he2e"].view, inp["key"].view, out_m1=m1.view, out_m2=m2.view,
                        out_selected=sel.view)
    torch.cuda.synchronize()
    for p, what in ((m1, "m1"), (m2, "m2"), (sel, "selected")):
        p.check(what, written=True)
    inputs_untouched()
    assert same_bits(m1.view, s["m1"]) and same_bits(m2.view, s["m2"]) and same_bits(sel.view, s["sel"])
    # apply, in place on copies
    pos, Q, faces = (Padded(dev, data=s[k]) for k in ("pos", "Q", "faces"))
    vmap = Padded(dev, data=np.arange(V, dtype=np.int32))
    dead = Padded(dev, shape=(F,), dtype=torch.uint8)
    ops.decimate_apply(pos.view, Q.view, faces.view, topo, inp["edges"].view, inp["cand"].view, inp["kept"].view, vmap.view,
                       out_face_dead=dead.view)
    torch.cuda.synchronize()
    for p, what in ((pos, "positions"), (Q, "quadrics"), (faces, "faces"), (vmap, "vertex map"), (dead, "dead faces")):
        p.check(what, written=True)
    inputs_untouched()
    assert same_bits(pos.view, s["pos2"]) and same_bits(Q.view, s["Q2"]) and same_bits(faces.view, s["faces2"])
    assert same_bits(vmap.view, s["map2"]) and same_bits(dead.view, s["dead"]) and s["dead"].sum() == 2 * s["kept"].shape[0]


_cpu_runs = {}


def cpu_run(key, v, f, target):
    """The numpy-backend run of decimate_mesh, once per case."""
    from actionmesh_amd import mesh_decimate as MD
    if key not in _cpu_runs:
        _cpu_runs[key] = MD.decimate_mesh(v, f, target, return_map=True, return_rounds=True, backend=R.NumpyBackend())
    return _cpu_runs[key]


def assert_device_equals_cpu(dev, key, v, f, target, runs=1):
    from actionmesh_amd import mesh_decimate as MD
    want = cpu_run(key, v, f, target)
    for _ in range(runs):
        got = MD.decimate_mesh(v.to(dev), f.to(dev), target, return_map=True, return_rounds=True)
        assert got[3] == want[3]
        for g, w in zip(got[:3], want[:3]):
            assert g.device.type == "cuda" and same_bits(g, w.numpy())
    return want


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(MESHES))
def test_whole_loop_equals_the_restatement(dev, name, dtype):
    make, target = MESHES[name]
    v, f = make()
    v, f = torch.from_numpy(v).to(dtype), torch.from_numpy(f)
    nv, nf, _, _ = assert_device_equals_cpu(dev, (name, dtype), v, f, target, runs=2)
    assert nf.shape[0] in (target, target - 1) and nv.dtype == dtype
    R.check_closed_manifold(nv.double().numpy(), nf.numpy(), R.euler(v.shape[0], f.numpy()))


@pytest.mark.parametrize("case", ["hub", "fin", "grid", "glued", "tetrahedron"])
def test_edge_cases_equal_the_restatement(dev, case):
    make, target = {"hub": (R.hub, 40), "fin": (lambda: R.finned_sphere()[:2], 100), "grid": (lambda: R.grid(12), 100),
                    "glued": (R.glued_tetrahedra, 2), "tetrahedron": (R.tetrahedron, 2)}[case]
    v, f = make()
    nv, nf, vmap, _ = assert_device_equals_cpu(dev, case, torch.from_numpy(v), torch.from_numpy(f), target)
    if case in ("glued", "tetrahedron"):
        assert nf.shape[0] == f.shape[0] > target
    if case == "grid":
        assert (nv[:, 2] == 0).all() and abs(R.face_areas(nv.numpy(), nf.numpy()).sum() - 121.0) <= 1e-12


def test_at_or_below_target_is_returned_as_it_is(dev):
    from actionmesh_amd import mesh_decimate as MD
    v, f = R.icosphere(1)
    tv, tf = torch.from_numpy(v).float().to(dev), torch.from_numpy(f).to(dev)
    nv, nf = MD.decimate_mesh(tv, tf, f.shape[0])
    assert nv is tv and nf is tf


@pytest.mark.parametrize("what", ["offset past 3F", "corner of another vertex", "corner past 3F", "face index", "edge table", "kept index"])
def test_corrupted_tables_raise_through_the_flag(dev, what):
    """No index is used as an address: the call returns, nothing outside the outputs is written, and the flag raises."""
    from actionmesh_amd import ops
    s = first_round(*R.icosphere(2))
    V, F, E = s["V"], s["faces"].shape[0], s["edges"].shape[0]
    if what == "offset past 3F":
        s["offsets"][5] = 3 * F + 7
    elif what == "corner of another vertex":
        a, b = s["offsets"][3], s["offsets"][9]
        s["corners"][a], s["corners"][b] = s["corners"][b], s["corners"][a]
    elif what == "corner past 3F":
        s["corners"][4] = 3 * F + 100
    elif what == "face index":
        s["faces"][2, 1] = V + 5
    elif what == "edge table":
        s["he2e"][0:3 * F:7] = E + 3
        s["edges"][1, 0] = V + 9
    elif what == "kept index":
        s["kept"][0] = E
    inp = {k: Padded(dev, data=s[k]) for k in ("pos", "faces", "offsets", "corners", "edges", "he2e", "count", "Q", "cand", "key", "kept")}
    topo = Topology(inp["offsets"].view, inp["corners"].view)
    outs = []

    def out(shape, dtype):
        outs.append(Padded(dev, shape=shape, dtype=dtype))
        return outs[-1].view

    calls = {
        "quadrics": lambda: ops.decimate_quadrics(inp["pos"].view, inp["faces"].view, topo, out=out((V, 10), torch.float64)),
        "edges": lambda: ops.decimate_edges(inp["pos"].view, inp["Q"].view, inp["faces"].view, topo, inp["edges"].view, inp["he2e"].view,
                                            inp["count"].view, out_positions=out((E, 3), torch.float64), out_cost=out((E,), torch.float64),
                                            out_key=out((E,), torch.int64)),
        "select": lambda: ops.decimate_select(V, inp["faces"].view, topo, inp["edges"].view, inp["he2e"].view, inp["key"].view,
                                              out_m1=out((V,), torch.int64), out_m2=out((V,), torch.int64), out_selected=out((E,), torch.uint8)),
        "apply": lambda: ops.decimate_apply(inp["pos"].view.clone(), inp["Q"].view.clone(), inp["faces"].view.clone(), topo, inp["edges"].view,
                                            inp["cand"].view, inp["kept"].view, out((V,), torch.int32), out_face_dead=out((F,), torch.uint8)),
    }
    raising = {"edge table": ("edges", "select"), "kept index": ("apply",)}.get(what, ("quadrics", "edges", "select"))
    for name in raising:
        with pytest.raises(ValueError, match="decimate_" + name):
            calls[name]()
    torch.cuda.synchronize()
    for p in outs:
        p.check("an output", written=True)
    for k, p in inp.items():
        p.check(k)


def test_decimate_mesh_raises_on_a_bad_face_index(dev):
    from actionmesh_amd import mesh_decimate as MD
    v, f = R.icosphere(1)
    f[5, 1] = v.shape[0]
    with pytest.raises(ValueError, match="outside"):
        MD.decimate_mesh(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), 20)


def test_process_mesh_decimates_on_the_device(dev):
    """clean-up -> decimate_mesh -> remove_floaters: a sphere and a small far component that the threshold removes."""
    from actionmesh_amd import mesh_cleanup, mesh_decimate as MD, mesh_prep as MP
    v, f = R.icosphere(3)
    v2, f2 = R.icosphere(0)
    tv = torch.from_numpy(np.concatenate((v, v2 * 0.2 + 5.0))).float().to(dev)
    tf = torch.from_numpy(np.concatenate((f, f2 + v.shape[0]))).to(dev)
    got = MP.process_mesh(tv, tf, face_decimation=300, floaters_threshold=0.5, decimation="hip")
    mid = MD.decimate_mesh(tv, tf, 300)
    want = mesh_cleanup.remove_floaters(*mid, threshold=0.5)
    assert mid[1].shape[0] in (300, 299) and want[1].shape[0] < mid[1].shape[0]
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(NotImplementedError, match="face_decimation"):
        MP.process_mesh(tv, tf, face_decimation=300)


@pytest.mark.parametrize("name", ["random-7x300", "icosphere3"])
def test_edge_tables_on_the_device_equal_the_cpu_tables(dev, name):
    """`mesh_topology.EdgeTables` is torch plumbing that runs wherever its faces are: `torch.unique`, or with `with_order` a stable
    sort, `unique_consecutive` and a scatter.  The device must give the CPU's tables in every field, both ways - for a 300-face array
    over 7 vertices (every edge many times, repeated indices within a face) and a small closed mesh (every edge twice)."""
    from actionmesh_amd.mesh_topology import EdgeTables
    if name == "random-7x300":
        faces, V = np.random.default_rng(11).integers(0, 7, (300, 3)), 7
    else:
        v, faces = R.icosphere(3)
        V = len(v)
    faces = torch.from_numpy(np.ascontiguousarray(faces))
    for n_vertices, with_order in ((V, False), (V, True), (None, True)):
        want, got = EdgeTables(faces, n_vertices, with_order), EdgeTables(faces.to(dev), n_vertices, with_order)
        for field in ("edges", "half_edge_to_edge", "edge_count") + (("order",) if with_order else ()):
            a, b = getattr(want, field), getattr(got, field)
            assert b.device.type == "cuda" and a.dtype == b.dtype and torch.equal(a, b.cpu()), (field, n_vertices, with_order)
