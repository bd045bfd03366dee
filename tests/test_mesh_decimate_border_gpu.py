"""Border collapses on the device (am_decimate_border_quadrics, am_decimate_border_edges) against the numpy restatement of the header
(tests/_decimate_border_ref.py), bit for bit: each kernel on the first-round state of the smallest meshes on which every case of the
topology rule occurs - every output in a sentinel-padded buffer and every input in a poisoned one, as tests/test_mesh_decimate_gpu.py
does, whose `Padded` this file uses -, then am_decimate_select / am_decimate_apply on that state, the whole loop, closed meshes against
`borders="fixed"`, the flag on corrupted tables, and a clipped iso-surface through clean-up and decimation."""
import numpy as np
import pytest
import torch

import _decimate_border_ref as B
import _decimate_ref as R
from test_mesh_decimate_gpu import Padded, Topology, same_bits

pytestmark = pytest.mark.gpu

FIRST_ROUND = {"grid5": lambda: R.grid(5), "cylinder8x4": lambda: B.open_cylinder(8, 4), "half_icosphere2": lambda: B.half_icosphere(2),
               "holes7": lambda: B.holes_grid(7), "ear": lambda: B.ear_disc()[:2], "strip": B.strip, "bow_tie": lambda: B.bow_tie()[:2]}
LOOPS = {"grid12": (lambda: R.grid(12), 40), "half_icosphere3": (lambda: B.half_icosphere(3), 60),
         "cylinder16x8": (lambda: B.open_cylinder(16, 8), 64)}
TABLES = ("pos", "faces", "offsets", "corners", "edges", "he2e", "count", "Q", "cand", "key")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from actionmesh_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def first_round(v, f, border_weight=1.0):
    """The first round of the restatement with border collapses: every table, every kernel's result."""
    V = v.shape[0]
    s = dict(V=V, pos=v.astype(np.float64), faces=f.astype(np.int32))
    s["offsets"], s["corners"] = R.np_topology(s["faces"], V)
    s["edges"], s["he2e"], s["count"] = R.np_edges(s["faces"], V)
    s["Q"] = B.ref_border_quadrics(s["pos"], s["faces"], s["offsets"], s["corners"], s["he2e"], s["count"], border_weight)
    s["cand"], s["cost"], s["key"] = B.ref_border_edges(s["pos"], s["Q"], s["faces"], s["offsets"], s["corners"], s["edges"], s["he2e"],
                                                        s["count"])
    s["m1"], s["m2"], s["sel"] = R.ref_select(V, s["edges"], s["key"])
    s["kept"] = np.nonzero(s["sel"])[0].astype(np.int32)[::-1].copy()           # any order
    s["pos2"], s["Q2"], s["faces2"], s["map2"] = s["pos"].copy(), s["Q"].copy(), s["faces"].copy(), np.arange(V, dtype=np.int32)
    if s["kept"].size:
        s["dead"] = R.ref_apply(s["pos2"], s["Q2"], s["faces2"], s["offsets"], s["corners"], s["edges"], s["cand"], s["kept"], s["map2"])
    return s


@pytest.mark.parametrize("weight", [1.0, 0.37], ids=["w1", "w0.37"])
@pytest.mark.parametrize("name", list(FIRST_ROUND))
def test_each_kernel_bit_identical_inside_guards(dev, name, weight):
    from actionmesh_amd import ops
    s = first_round(*FIRST_ROUND[name](), border_weight=weight)
    V, F, E = s["V"], s["faces"].shape[0], s["edges"].shape[0]
    inp = {k: Padded(dev, data=s[k]) for k in TABLES}
    topo = Topology(inp["offsets"].view, inp["corners"].view)

    def inputs_untouched():
        for k, p in inp.items():
            p.check(k)

    # quadrics: the ten fp64 bit patterns of every vertex
    q = Padded(dev, shape=(V, 10), dtype=torch.float64)
    assert ops.decimate_border_quadrics(inp["pos"].view, inp["faces"].view, topo, inp["he2e"].view, inp["count"].view, weight,
                                        out=q.view) is q.view
    torch.cuda.synchronize()
    q.check("quadrics", written=True)
    inputs_untouched()
    assert same_bits(q.view, s["Q"])
    assert not same_bits(q.view, R.ref_quadrics(s["pos"], s["faces"], s["offsets"], s["corners"]))         # the border planes are in
    # edges
    cand, cost, key = (Padded(dev, shape=sh, dtype=dt) for sh, dt in (((E, 3), torch.float64), ((E,), torch.float64), ((E,), torch.int64)))
    ops.decimate_border_edges(inp["pos"].view, inp["Q"].view, inp["faces"].view, topo, inp["edges"].view, inp["he2e"].view,
                              inp["count"].view, out_positions=cand.view, out_cost=cost.view, out_key=key.view)
    torch.cuda.synchronize()
    for p, what in ((cand, "candidates"), (cost, "cost"), (key, "key")):
        p.check(what, written=True)
    inputs_untouched()
    assert same_bits(cand.view, s["cand"]) and same_bits(cost.view, s["cost"]) and same_bits(key.view, s["key"])
    if name == "strip":
        assert (s["key"] == R.NO_KEY).all()
        return
    border = s["count"] == 1
    assert (s["key"][border] != R.NO_KEY).any() and ((s["key"] != R.NO_KEY) & ~border).any()
    # select and apply as they are, on this state
    m1, m2, sel = (Padded(dev, shape=sh, dtype=dt) for sh, dt in (((V,), torch.int64), ((V,), torch.int64), ((E,), torch.uint8)))
    ops.decimate_select(V, inp["faces"].view, topo, inp["edges"].view, inp["he2e"].view, inp["key"].view, out_m1=m1.view, out_m2=m2.view,
                        out_selected=sel.view)
    torch.cuda.synchronize()
    for p, what in ((m1, "m1"), (m2, "m2"), (sel, "selected")):
        p.check(what, written=True)
    inputs_untouched()
    assert same_bits(m1.view, s["m1"]) and same_bits(m2.view, s["m2"]) and same_bits(sel.view, s["sel"]) and s["kept"].size
    kept = Padded(dev, data=s["kept"])
    pos, Q, faces = (Padded(dev, data=s[k]) for k in ("pos", "Q", "faces"))
    vmap = Padded(dev, data=np.arange(V, dtype=np.int32))
    dead = Padded(dev, shape=(F,), dtype=torch.uint8)
    ops.decimate_apply(pos.view, Q.view, faces.view, topo, inp["edges"].view, inp["cand"].view, kept.view, vmap.view, out_face_dead=dead.view)
    torch.cuda.synchronize()
    for p, what in ((pos, "positions"), (Q, "quadrics"), (faces, "faces"), (vmap, "vertex map"), (dead, "dead faces")):
        p.check(what, written=True)
    inputs_untouched()
    kept.check("kept")
    assert same_bits(pos.view, s["pos2"]) and same_bits(Q.view, s["Q2"]) and same_bits(faces.view, s["faces2"])
    assert same_bits(vmap.view, s["map2"]) and same_bits(dead.view, s["dead"]) and s["dead"].sum() == s["count"][s["kept"]].sum()


_cpu_runs = {}


def cpu_run(name):
    """The numpy-backend run of one whole-loop case, once."""
    from actionmesh_amd import mesh_decimate as MD
    if name not in _cpu_runs:
        make, target = LOOPS[name]
        v, f = make()
        _cpu_runs[name] = (v, f, MD.decimate_mesh(torch.from_numpy(v), torch.from_numpy(f), target, return_map=True, return_rounds=True,
                                                  backend=B.NumpyBorderBackend(), borders="collapse"))
    return _cpu_runs[name]


@pytest.mark.parametrize("name", list(LOOPS))
def test_whole_loop_equals_the_restatement_twice(dev, name):
    from actionmesh_amd import mesh_decimate as MD
    v, f, want = cpu_run(name)
    target = LOOPS[name][1]
    for _ in range(2):
        got = MD.decimate_mesh(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), target, return_map=True, return_rounds=True,
                               borders="collapse")
        assert got[3] == want[3]
        for g, w in zip(got[:3], want[:3]):
            assert g.device.type == "cuda" and same_bits(g, w.numpy())
    assert want[1].shape[0] in (target, target - 1)
    B.check_open_manifold(want[0].numpy(), want[1].numpy(), R.euler(v.shape[0], f), len(B.border_loops(f)))


def test_closed_mesh_equals_the_fixed_mode_bit_for_bit(dev):
    from actionmesh_amd import mesh_decimate as MD
    v, f = R.icosphere(3)
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    fixed = MD.decimate_mesh(tv, tf, 200, return_map=True, return_rounds=True)
    moved = MD.decimate_mesh(tv, tf, 200, return_map=True, return_rounds=True, borders="collapse")
    assert fixed[3] == moved[3] and all(same_bits(a, b.cpu().numpy()) for a, b in zip(moved[:3], fixed[:3]))


def test_closed_mesh_kernels_equal_the_fixed_mode_kernels_bit_for_bit(dev):
    """Kernel by kernel what the loop test above shows end to end: without a border the two instantiations of the gather and of the edge
    evaluation give the same bits, whatever the border weight."""
    from actionmesh_amd import ops
    v, f = R.icosphere(2)
    assert f.shape[0] == 320
    V = v.shape[0]
    offsets, corners = R.np_topology(f.astype(np.int32), V)
    edges, he2e, count = R.np_edges(f.astype(np.int32), V)
    assert (count == 2).all()
    pos, faces, edges, he2e, count = (torch.from_numpy(np.ascontiguousarray(x)).to(dev)
                                      for x in (v.astype(np.float64), f.astype(np.int32), edges, he2e, count))
    topo = Topology(torch.from_numpy(offsets).to(dev), torch.from_numpy(corners).to(dev))
    q = ops.decimate_quadrics(pos, faces, topo)
    assert same_bits(ops.decimate_border_quadrics(pos, faces, topo, he2e, count, border_weight=0.37), q.cpu().numpy())
    fixed = ops.decimate_edges(pos, q, faces, topo, edges, he2e, count)
    moved = ops.decimate_border_edges(pos, q, faces, topo, edges, he2e, count)
    for a, b in zip(moved, fixed):          # candidates, cost, key
        assert same_bits(a, b.cpu().numpy())
    assert (fixed[2] != R.NO_KEY).any()


@pytest.mark.parametrize("what", ["offset out of order", "corner of another vertex", "edge with u > v", "half-edge entry out of range",
                                  "edge_count 0", "edge_count 7"])
def test_corrupted_tables_raise_through_the_flag(dev, what):
    """Bad indices that the kernels refuse by comparison: the call returns, nothing outside the outputs is written, the flag raises."""
    from actionmesh_amd import ops
    s = first_round(*B.half_icosphere(2))
    V, F, E = s["V"], s["faces"].shape[0], s["edges"].shape[0]
    raising = ("quadrics", "edges")
    if what == "offset out of order":
        s["offsets"][5] = s["offsets"][7] + 1
    elif what == "corner of another vertex":
        a, b = s["offsets"][3], s["offsets"][9]
        s["corners"][a], s["corners"][b] = s["corners"][b], s["corners"][a]
    elif what == "edge with u > v":
        s["edges"][4] = s["edges"][4, ::-1].copy()
        raising = ("edges",)                    # the quadrics do not read the edge list
    elif what == "half-edge entry out of range":
        s["he2e"][0:3 * F:7] = E + 3
        s["he2e"][5] = -1
    elif what == "edge_count 0":
        s["count"][np.nonzero(s["count"] == 1)[0][0]] = 0
        s["count"][np.nonzero(s["count"] == 2)[0][0]] = 0
    elif what == "edge_count 7":
        s["count"][np.nonzero(s["count"] == 2)[0][3]] = 7
        raising = ("edges",)                    # to the quadrics 7 is "not a border"; the edges see that two faces hold the edge
    inp = {k: Padded(dev, data=s[k]) for k in TABLES}
    topo = Topology(inp["offsets"].view, inp["corners"].view)
    outs = []

    def out(shape, dtype):
        outs.append(Padded(dev, shape=shape, dtype=dtype))
        return outs[-1].view

    calls = {
        "quadrics": lambda: ops.decimate_border_quadrics(inp["pos"].view, inp["faces"].view, topo, inp["he2e"].view, inp["count"].view,
                                                         out=out((V, 10), torch.float64)),
        "edges": lambda: ops.decimate_border_edges(inp["pos"].view, inp["Q"].view, inp["faces"].view, topo, inp["edges"].view,
                                                   inp["he2e"].view, inp["count"].view, out_positions=out((E, 3), torch.float64),
                                                   out_cost=out((E,), torch.float64), out_key=out((E,), torch.int64)),
    }
    for name in raising:
        with pytest.raises(ValueError, match="decimate_border_" + name):
            calls[name]()
    torch.cuda.synchronize()
    for p in outs:
        p.check("an output", written=True)
    for k, p in inp.items():
        p.check(k)


def test_a_clipped_isosurface_reaches_the_target(dev):
    """A sphere of radius 0.8 in a box of half-extent 0.6 along z: the iso-surface is a band with two border loops.  Clean-up, then
    400 faces with border collapses; where `borders="fixed"` stops is printed, not asserted."""
    from actionmesh_amd import isosurface as ISO, mesh_decimate as MD, mesh_prep as MP
    n = 33
    x, z = torch.linspace(-1.0, 1.0, n, device=dev), torch.linspace(-0.6, 0.6, n, device=dev)
    values = 0.8 - torch.sqrt(x[:, None, None] ** 2 + x[None, :, None] ** 2 + z[None, None, :] ** 2)
    v, f = ISO.extract_isosurface(values.contiguous(), bounds=(-1.0, -1.0, -0.6, 1.0, 1.0, 0.6))
    cv, cf = MP.merge_and_clean_mesh(v, f)[:2]
    before = (cv.double().cpu().numpy(), cf.cpu().numpy())
    B.check_open_manifold(*before, 0, 2)
    assert cf.shape[0] > 2000
    nv, nf = MD.decimate_mesh(cv, cf, 400, borders="collapse")
    assert nf.shape[0] in (400, 399)
    B.check_open_manifold(nv.double().cpu().numpy(), nf.cpu().numpy(), 0, 2)
    print(f"clipped sphere: {cf.shape[0]} faces -> {nf.shape[0]} with borders='collapse', "
          f"{MD.decimate_mesh(cv, cf, 400)[1].shape[0]} with borders='fixed'")
