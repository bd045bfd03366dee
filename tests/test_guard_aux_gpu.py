"""Guard bands and exact workspaces of the auxiliary kernels - am_nn_search, am_render_normals, am_mask_refine, am_graph_components,
am_fps, am_image_resample, am_image_materialize, am_image_alpha_stats - called through the C ABI itself (the struct table of
actionmesh_amd/_lib.py, torch's current stream), at the smallest shapes that still cross a block, wave or tile edge.

Every output lies in an arena of sentinels (tests/_guard.py), every input in a poisoned one (NaN around floats, 0x5A5A5A5A around
indices, 0xA5 around bytes), the workspace in a uint8 arena of EXACTLY the bytes the entry point's query function returns, and that
count is what the library is told.  After the call every guard is untouched, every input holds the bits it held, and the values equal
the restatement the family's own test file uses.  Each case runs twice, the workspace interior once left at the sentinel and once
zeroed: a result may not depend on what the scratch held.  Declaring one byte less must fail on the host, name the size needed, and
launch nothing."""
import ctypes as C

import numpy as np
import pytest
import torch
from PIL import Image

import test_components_cpu as cc
import test_render_gpu as tr
from _guard import SENTINEL, Arena, Padded64
from actionmesh_amd import _lib as L
from actionmesh_amd import image_preprocess as IP
from actionmesh_amd.mesh_topology import MeshTopology
from test_fps_cpu import fps_restatement
from test_nn_plans_gpu import brute, nn_plan

pytestmark = pytest.mark.gpu

OUT64 = -7.25e300               # what an fp64 output holds before the call


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
    """A copy of `t` inside a poisoned arena; unchanged() holds every bit of it - values, gaps and guards - to what it was."""

    def __init__(self, t, dev, arena=None):
        self.a = Arena.flat_of(t.contiguous().to(dev)) if arena is None else arena
        self.ptr = self.a.view.data_ptr()
        self.before = self.a.bits.clone()

    def unchanged(self, what):
        assert torch.equal(self.a.bits, self.before), f"{what}: the input or its guards changed"


def out_arena(shape, dtype, dev):
    return Arena.flat(shape, dtype, dev)


def workspace(nbytes, dev, zero):
    """uint8 arena of exactly `nbytes`, its interior at the sentinel 0xA5 or zeroed"""
    a = Arena.flat((nbytes,), torch.uint8, dev)
    if zero:
        a.view.zero_()
    return a


def both_fills(run):
    """run(zero) -> {name: tensor}: once over a sentinel-filled and once over a zeroed workspace; the results must be the same bits"""
    first, second = run(False), run(True)
    assert first.keys() == second.keys()
    for k in first:
        assert torch.equal(first[k].view(torch.uint8), second[k].view(torch.uint8)), f"{k} depends on what the workspace held"
    return first


def refused(lib, status, need):
    assert status != 0, "a workspace one byte short was accepted"
    msg = lib.am_last_error().decode()
    assert "workspace" in msg and str(need) in msg, msg


# ---- am_nn_search ------------------------------------------------------------------------------------------------------------------
NN_PLANS = {(513, 7, 1): (1, 1), (2049, 257, 3): (1, 2), (5, 1025, 512): (4, 1)}        # (queries per thread, point splits)


@pytest.mark.parametrize("precise", [0, 1], ids=["fp32", "fp64"])
@pytest.mark.parametrize("P,Q,B", list(NN_PLANS))
def test_nn_search_guards(dev, lib, P, Q, B, precise):
    qpt, _, nsplit = nn_plan(P, Q, B)
    assert (qpt, nsplit) == NN_PLANS[(P, Q, B)]
    need = lib.am_nn_workspace_bytes(P, Q, B, precise)
    assert need == (((8 if precise else 4) + 4) * B * nsplit * Q if nsplit > 1 else 0)
    g = torch.Generator().manual_seed(P + Q)
    pts, qry = torch.randn((B, P, 3), generator=g), torch.randn((B, Q, 3), generator=g)
    pts[:, P - 1] = pts[:, 1]               # a duplicate in the last row: the lower index wins
    qry[:, Q - 1] = pts[:, 1]
    PA, QA = Input(pts, dev), Input(qry, dev)

    def args(idx, d2):
        a = L.AmNnArgs()
        a.points, a.n_points, a.points_bstride = PA.ptr, P, P * 3
        a.queries, a.n_queries, a.queries_bstride = QA.ptr, Q, Q * 3
        a.batch, a.precise, a.out_index, a.out_d2 = B, precise, idx.view.data_ptr(), d2.view.data_ptr()
        return a

    def outputs():
        return out_arena((B, Q), torch.int32, dev), (Padded64((B, Q), dev, OUT64) if precise else out_arena((B, Q), torch.float32, dev))

    def run(zero):
        idx, d2 = outputs()
        # no workspace needed: none at all for the four-queries plan, else 16 bytes that must stay as they are
        ws = None if need == 0 and qpt == 4 else workspace(need or 16, dev, zero)
        before = None if ws is None else ws.bits.clone()
        a = args(idx, d2)
        status = lib.am_nn_search(C.byref(a), None if ws is None else ws.view.data_ptr(), 0 if ws is None else ws.view.numel(), stream())
        assert status == 0, lib.am_last_error()
        torch.cuda.synchronize()
        idx.assert_untouched("out_index")
        d2.assert_untouched("out_d2", written=True) if precise else d2.assert_untouched("out_d2")
        if ws is not None:
            ws.assert_untouched("workspace")
            if need == 0:
                assert torch.equal(ws.bits, before), "a workspace that is not needed was written"
        PA.unchanged("points"), QA.unchanged("queries")
        return {"index": idx.view.clone(), "d2": d2.view.clone()}

    got = both_fills(run)
    ri, rd = brute(qry.numpy(), pts.numpy(), np.float64 if precise else np.float32)
    assert np.array_equal(got["index"].cpu().numpy(), ri)
    assert np.array_equal(got["d2"].cpu().numpy().view(np.uint8), rd.view(np.uint8))
    assert (got["index"][:, Q - 1] == 1).all()
    if need:
        idx, d2 = outputs()
        ws = workspace(need, dev, False)
        a = args(idx, d2)
        refused(lib, lib.am_nn_search(C.byref(a), ws.view.data_ptr(), need - 1, stream()), need)
        torch.cuda.synchronize()
        assert (idx.view == SENTINEL[torch.int32]).all() and (ws.view == 0xA5).all(), "something was launched"
        idx.assert_untouched("out_index"), ws.assert_untouched("workspace")


# ---- am_render_normals -----------------------------------------------------------------------------------------------------------
def _rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m = np.eye(3)
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def _cameras(n):
    """n variations of test_render_gpu.cam(): the unit ball stays in front of every one (view z >= 2 - 1)"""
    return [tr.cam(_rot(1, 2 * np.pi * k / n) @ _rot(0, 0.3 * (k % 3)), T=(0.05 * (k % 5), -0.03 * (k % 4), 2.0 + 0.1 * (k % 4)),
                   f=1.0 + 0.25 * (k % 3)) for k in range(n)]


def _ball_mesh(T, V, F, seed):
    """fp32 vertices (T, V, 3) inside the unit ball, F random faces of distinct vertices; the last vertex is on face 0"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(T, V, 3))
    v = d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.random((T, V, 1)) ** (1 / 3)
    f = np.stack([rng.choice(V, 3, replace=False) for _ in range(F)]).astype(np.int32)
    if V - 1 not in f[0]:
        f[0, 0] = V - 1
    return v.astype(np.float32), f


def _compare_image(got, ref, S):
    """one image against restate(): the comparisons and tolerances of test_render_gpu.check_against_restatement"""
    st = ref["stable"]
    assert np.array_equal(got["face"][st], ref["face"][st]), "face index differs on stable sub-pixels"
    covered = st & (ref["face"] >= 0)
    if covered.any():
        assert np.abs(got["bary"][covered] - ref["bary"][covered]).max() < 1e-4
    px = st.reshape(S, 2, S, 2).all((1, 3))
    assert np.array_equal(got["mask"][px], ref["mask"][px])
    if px.any():
        assert np.abs(got["normal"][px] - ref["normal"][px]).max() < 1e-4
        assert np.abs(got["rgba"][px].astype(np.int64) - ref["rgba8"][px]).max() <= 1
    return int(st.sum()), int(covered.sum())


RENDER_OUT = {"rgba": (torch.uint8, lambda S: (S, S, 4)), "mask": (torch.float32, lambda S: (S, S)),
              "normal": (torch.float32, lambda S: (S, S, 3)), "face": (torch.int32, lambda S: (2 * S, 2 * S)),
              "bary": (torch.float32, lambda S: (2 * S, 2 * S, 3))}


def _mesh_inputs(faces, V, dev):
    """faces (F, 3) int32 numpy -> the faces and the vertex -> corner CSR of MeshTopology, each in a poisoned arena"""
    topo = MeshTopology(torch.from_numpy(faces).to(dev), V)
    return tuple(Input(t, dev) for t in (topo.faces, topo.offsets, topo.corners))


def _render(lib, dev, VA, mesh, cams, T, V, F, S, names, zero, short=False, flag_bits=0):
    """One call on (faces, offsets, corners) = `mesh`; the flag word, in an arena of its own, must end at `flag_bits`."""
    Cn = len(cams)
    need = lib.am_render_workspace_bytes(T, V, F, Cn, S)
    assert need > 0
    outs = {k: out_arena((T, Cn) + RENDER_OUT[k][1](S), RENDER_OUT[k][0], dev) for k in names}
    ws = workspace(need, dev, zero)
    flag = out_arena((1,), torch.int32, dev)
    FA, OA, CA = mesh
    a = L.AmRenderArgs()
    a.verts, a.faces, a.offsets, a.corners, a.out_flag = VA.ptr, FA.ptr, OA.ptr, CA.ptr, flag.view.data_ptr()
    a.n_frames, a.n_verts, a.n_faces, a.n_cameras, a.image_size = T, V, F, Cn, S
    for k, cam in enumerate(cams):
        c = a.cameras[k]
        for i, x in enumerate(cam["R"].reshape(9).tolist()):
            c.R[i] = x
        for i, x in enumerate(cam["T"].tolist()):
            c.T[i] = x
        c.fx, c.fy = (float(x) for x in cam["focal_length"])
        c.px, c.py = (float(x) for x in cam["principal_point"])
    a.out_rgba = outs["rgba"].view.data_ptr()
    a.out_mask, a.out_normal = (outs[k].view.data_ptr() if k in outs else None for k in ("mask", "normal"))
    a.out_face, a.out_bary = (outs[k].view.data_ptr() if k in outs else None for k in ("face", "bary"))
    status = lib.am_render_normals(C.byref(a), ws.view.data_ptr(), need - 1 if short else need, stream())
    torch.cuda.synchronize()
    for k, o in outs.items():
        o.assert_untouched(k)
    ws.assert_untouched("workspace"), flag.assert_untouched("out_flag")
    VA.unchanged("vertices"), FA.unchanged("faces"), OA.unchanged("offsets"), CA.unchanged("corners")
    if short:
        refused(lib, status, need)
        assert (ws.view == 0xA5).all() and (outs["rgba"].view == 0xA5).all(), "something was launched"
        assert int(flag.view) == SENTINEL[torch.int32], "the flag was cleared although nothing may be launched"
        return None
    assert status == 0, lib.am_last_error()
    assert int(flag.view) == flag_bits, f"out_flag {int(flag.view)}, expected {flag_bits}"
    return {k: o.view.clone() for k, o in outs.items()}


@pytest.mark.parametrize("T,V,F,Cn,S", [(1, 3, 1, 1, 1), (2, 65, 129, 3, 17), (1, 1025, 300, 16, 8)])
def test_render_normals_guards(dev, lib, T, V, F, Cn, S):
    verts, faces = _ball_mesh(T, V, F, 1000 * V + F)
    cams = _cameras(Cn)
    VA, mesh = Input(torch.from_numpy(verts), dev), _mesh_inputs(faces, V, dev)
    common = (lib, dev, VA, mesh, cams, T, V, F, S)
    full = both_fills(lambda zero: _render(*common, tuple(RENDER_OUT), zero))
    alone = both_fills(lambda zero: _render(*common, ("rgba",), zero))
    assert torch.equal(alone["rgba"], full["rgba"]), "out_rgba depends on which optional outputs are asked for"
    host = {k: t.cpu().numpy() for k, t in full.items()}
    stable = covered = 0
    for t in range(T):
        for c in range(Cn):
            ref = tr.restate(verts[t].astype(np.float64), faces.astype(np.int64), cams[c], S)
            n_st, n_cov = _compare_image({k: h[t, c] for k, h in host.items()}, ref, S)
            stable, covered = stable + n_st, covered + n_cov
    if S > 1:
        assert stable > 0.5 * T * Cn * 4 * S * S and covered > 0, (stable, covered)
    if S == 17:                     # every image of the batch equals the call that renders it alone, bit for bit
        for t in range(T):
            Vt = Input(torch.from_numpy(verts[t: t + 1]), dev)
            for c in range(Cn):
                single = _render(lib, dev, Vt, mesh, cams[c: c + 1], 1, V, F, S, tuple(RENDER_OUT), False)
                for k in full:
                    assert torch.equal(single[k][0, 0].view(torch.uint8), full[k][t, c].view(torch.uint8)), (k, t, c)
    _render(*common, tuple(RENDER_OUT), False, short=True)


def test_render_normals_reports_a_foreign_csr(dev, lib):
    """The octahedron of test_render_gpu, one camera, S = 8.  A clean call leaves the flag at 0.  Offsets that descend at one vertex,
    and a corner listed under a vertex it does not name, are each answered with AM_OK and AM_MESH_BAD_CSR alone, and nothing outside
    the outputs, the workspace and the flag word is written."""
    verts, faces = tr.octahedron((0.0, 0.0, 0.0), 0.5)
    V, F, S = len(verts), len(faces), 8
    VA = Input(torch.from_numpy(verts[None].astype(np.float32)), dev)
    FA, OA, CA = _mesh_inputs(faces.astype(np.int32), V, dev)
    assert OA.a.view.tolist() == [0, 4, 8, 12, 16, 20, 24]                  # four faces on every vertex
    common = (lib, dev, VA)
    shape = ([tr.cam()], 1, V, F, S, tuple(RENDER_OUT), False)
    clean = _render(*common, (FA, OA, CA), *shape, flag_bits=0)
    assert int((clean["face"] >= 0).sum()) > 0
    offsets = OA.a.view.clone()
    offsets[3] = 6                                                          # vertex 2: [8, 6)
    _render(*common, (FA, Input(offsets, dev), CA), *shape, flag_bits=L.MESH_BAD_CSR)
    corners = CA.a.view.clone()
    corners[0] = corners[4]                                                 # a corner of vertex 1 in the list of vertex 0
    assert int(FA.a.view.reshape(-1)[corners[0]]) == 1
    _render(*common, (FA, OA, Input(corners, dev)), *shape, flag_bits=L.MESH_BAD_CSR)


# ---- am_mask_refine --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optional", [True, False], ids=["labels+stats", "mask-only"])
@pytest.mark.parametrize("threshold", [-1, 100], ids=["otsu", "fixed"])
@pytest.mark.parametrize("T,H,W", [(1, 1, 1), (2, 33, 47), (1, 64, 65)])
def test_mask_refine_guards(dev, lib, T, H, W, threshold, optional):
    rng = np.random.default_rng(H * W + T)
    frames = np.where(rng.random((T, H, W)) < 0.45, rng.integers(120, 256, (T, H, W)), rng.integers(0, 90, (T, H, W))).astype(np.uint8)
    min_size = 1 if H == 1 else 4
    need = lib.am_mask_refine_workspace_bytes(T, H, W)
    a16 = lambda b: (b + 15) // 16 * 16
    assert need == 2 * a16(T * H * W * 4) + a16(T * 256 * 4) + a16(T * 4)          # am_mask_refine_workspace_bytes
    MA = Input(torch.from_numpy(frames), dev)

    def call(zero, short=False):
        out = out_arena((T, H, W), torch.uint8, dev)
        lab = out_arena((T, H, W), torch.int32, dev) if optional else None
        stats = out_arena((T, 4), torch.int32, dev) if optional else None
        ws = workspace(need, dev, zero)
        a = L.AmMaskRefineArgs()
        a.mask, a.n_frames, a.height, a.width, a.min_size, a.threshold = MA.ptr, T, H, W, min_size, threshold
        a.out_mask = out.view.data_ptr()
        a.out_labels, a.out_stats = (None, None) if not optional else (lab.view.data_ptr(), stats.view.data_ptr())
        a.workspace, a.workspace_bytes = ws.view.data_ptr(), need - 1 if short else need
        status = lib.am_mask_refine(C.byref(a), stream())
        torch.cuda.synchronize()
        for o, what in ((out, "out_mask"), (lab, "out_labels"), (stats, "out_stats"), (ws, "workspace")):
            if o is not None:
                o.assert_untouched(what)
        MA.unchanged("mask")
        if short:
            refused(lib, status, need)
            assert (ws.view == 0xA5).all() and (out.view == 0xA5).all(), "something was launched"
            return None
        assert status == 0, lib.am_last_error()
        res = {"mask": out.view.clone()}
        if optional:
            res.update(labels=lab.view.clone(), stats=stats.view.clone())
        return res

    got = {k: t.cpu().numpy() for k, t in both_fills(call).items()}
    for t in range(T):
        want_out, want_lab, want_stats = cc.refine_restatement(frames[t], min_size, None if threshold < 0 else threshold)
        assert np.array_equal(got["mask"][t], want_out)
        if optional:
            assert np.array_equal(got["labels"][t], want_lab) and got["stats"][t].tolist() == want_stats.tolist()
    call(False, short=True)


# ---- am_graph_components ---------------------------------------------------------------------------------------------------------
def _graph_cases():
    rng = np.random.default_rng(5)
    e = rng.integers(0, 257, (100, 2))
    loops = np.stack([np.arange(0, 100), np.arange(0, 100)], 1)
    mixed = np.concatenate([e, e[::-1, ::-1], loops])                              # 300 edges: duplicates (reversed) and self-loops
    path = np.stack([np.arange(4095), np.arange(1, 4096)], 1)[rng.permutation(4095)]
    return {"single-node": (1, np.zeros((0, 2), np.int64)), "257-nodes": (257, mixed), "4096-path": (4096, path)}


@pytest.mark.parametrize("case", list(_graph_cases()))
def test_graph_components_guards(dev, lib, case):
    n, edges = _graph_cases()[case]
    E = len(edges)
    assert (n, E) in ((1, 0), (257, 300), (4096, 4095))
    need = lib.am_graph_components_workspace_bytes(n, E)
    assert need == (n * 4 + 15) // 16 * 16
    EA = Input(torch.from_numpy(edges.astype(np.int32)), dev) if E else None

    def call(zero, short=False):
        lab, size, flag = out_arena((n,), torch.int32, dev), out_arena((n,), torch.int32, dev), out_arena((1,), torch.int32, dev)
        ws = workspace(need, dev, zero)
        a = L.AmGraphArgs()
        a.n_nodes, a.n_edges, a.edges = n, E, (EA.ptr if E else None)
        a.out_label, a.out_size, a.out_flag = lab.view.data_ptr(), size.view.data_ptr(), flag.view.data_ptr()
        a.workspace, a.workspace_bytes = ws.view.data_ptr(), need - 1 if short else need
        status = lib.am_graph_components(C.byref(a), stream())
        torch.cuda.synchronize()
        for o, what in ((lab, "out_label"), (size, "out_size"), (flag, "out_flag"), (ws, "workspace")):
            o.assert_untouched(what)
        if E:
            EA.unchanged("edges")
        if short:
            refused(lib, status, need)
            assert (ws.view == 0xA5).all() and (lab.view == SENTINEL[torch.int32]).all(), "something was launched"
            return None
        assert status == 0, lib.am_last_error()
        return {"label": lab.view.clone(), "size": size.view.clone(), "flag": flag.view.clone()}

    got = both_fills(call)
    want_lab, want_size = cc.graph_restatement(n, edges)
    assert np.array_equal(got["label"].cpu().numpy(), want_lab) and np.array_equal(got["size"].cpu().numpy(), want_size)
    assert got["flag"].tolist() == [0]
    call(False, short=True)


# ---- am_fps ------------------------------------------------------------------------------------------------------------------------
FPS_RESIDENT = 8192             # csrc/am_fps.hip: beyond it the streaming form, which needs the workspace


@pytest.mark.parametrize("B,N,K,D,dd", [(2, 65, 65, 3, 3), (1, 2049, 40, 8, 6), (2, 8193, 33, 3, 3), (1, 8194, 17, 8, 8)])
def test_fps_guards(dev, lib, B, N, K, D, dd):
    need = lib.am_fps_workspace_bytes(N, B, dd)
    npad = (N + 3) // 4 * 4
    assert need == (4 * B * npad * (1 + dd) if N > FPS_RESIDENT else 0)             # am_fps_workspace_bytes
    stride, bstride = D + 3, N * (D + 3) + 7                                       # a point stride above D, a batch stride above N * stride
    rng = np.random.default_rng(N + D)
    data = rng.normal(size=(B, N, D)).astype(np.float32)
    wide = np.full((B, N, stride), np.nan, np.float32)
    wide[..., :D] = data
    arena = Arena(B, N * stride, torch.float32, dev, ld=bstride, guard_rows=2)
    arena.view.copy_(torch.from_numpy(wide.reshape(B, N * stride)))
    PA = Input(None, dev, arena=arena)
    start = np.array([5, N - 1][:B], np.int32)
    SA = Input(torch.from_numpy(start), dev)

    def call(zero, short=False):
        idx, dist = out_arena((B, K), torch.int32, dev), out_arena((B, K), torch.float32, dev)
        ws = workspace(need, dev, zero) if need else None
        a = L.AmFpsArgs()
        a.points, a.dtype, a.batch, a.n_points = PA.ptr, L.FPS_F32, B, N
        a.dims, a.dist_dims, a.batch_stride, a.point_stride, a.n_samples = D, dd, bstride, stride, K
        a.start_idx, a.out_index, a.out_dist = SA.ptr, idx.view.data_ptr(), dist.view.data_ptr()
        a.workspace, a.workspace_bytes = (ws.view.data_ptr() if need else None), (need - 1 if short else need)
        status = lib.am_fps(C.byref(a), stream())
        torch.cuda.synchronize()
        idx.assert_untouched("out_index"), dist.assert_untouched("out_dist")
        if ws is not None:
            ws.assert_untouched("workspace")
        PA.unchanged("points"), SA.unchanged("start_idx")
        if short:
            refused(lib, status, need)
            assert (ws.view == 0xA5).all() and (idx.view == SENTINEL[torch.int32]).all(), "something was launched"
            return None
        assert status == 0, lib.am_last_error()
        return {"index": idx.view.clone(), "dist": dist.view.clone()}

    got = {k: t.cpu().numpy() for k, t in both_fills(call).items()}
    for b in range(B):
        want_idx, want_dist = fps_restatement(data[b], K, int(start[b]), dd)
        assert np.array_equal(got["index"][b], want_idx), b
        assert np.array_equal(got["dist"][b].view(np.uint32), want_dist.view(np.uint32)), b
    if need:
        call(False, short=True)


# ---- am_image_* --------------------------------------------------------------------------------------------------------------------
def _frame_array(sources, dst_offsets=None):
    frames = (L.AmImageFrame * len(sources))()
    for i, s in enumerate(sources):
        f = frames[i]
        f.src_offset, f.src_w, f.src_h = s.src_offset, s.src_w, s.src_h
        f.x0, f.y0, f.w, f.h, f.pad_x, f.pad_y = s.x0, s.y0, s.w, s.h, s.pad_x, s.pad_y
        if dst_offsets is not None:
            f.dst_offset = dst_offsets[i]
    return frames


def _padded(stored, s, fill=255):
    """the virtual source image of one frame: the window of the stored (h, w, 3) image inside pad_x / pad_y of `fill`"""
    win = stored[s.y0: s.y0 + s.h, s.x0: s.x0 + s.w]
    return np.pad(win, ((s.pad_y, s.pad_y), (s.pad_x, s.pad_x), (0, 0)), constant_values=fill)


@pytest.mark.parametrize("out_w,out_h", [(255, 3), (256, 4)])
def test_image_resample_guards(dev, lib, out_w, out_h):
    """Two RGB frames of different geometry in one call: a 20 x 15 window of a 23 x 17 frame inside padding, and a whole 9 x 7 frame
    whose last byte is the last byte of the source - the arena behind it is poison, so the last-bytes path of the RGB fetch is what
    keeps the guard unread (a read past the end cannot be seen directly; the values would only change if it were used)."""
    rng = np.random.default_rng(out_w)
    img = [rng.integers(0, 256, (17, 23, 3), dtype=np.uint8), rng.integers(0, 256, (7, 9, 3), dtype=np.uint8)]
    off1 = (img[0].size + 3) // 4 * 4
    src_bytes = off1 + img[1].size
    assert src_bytes % 4 != 0                                                      # the last pixel cannot be read as two aligned words
    src = np.full(src_bytes, 0xA5, np.uint8)
    src[: img[0].size], src[off1:] = img[0].reshape(-1), img[1].reshape(-1)
    sources = [IP._Source(0, 23, 17, 2, 1, 20, 15, 1, 2), IP._Source(off1, 9, 7, 0, 0, 9, 7)]
    frames, taps, _ = IP._describe(sources, [(out_w, out_h, 0, 0)] * 2, (out_h, out_w))
    max_rows = max(f.n_rows for f in frames)
    need = lib.am_image_resample_workspace_bytes(2, max_rows, out_w)
    assert need == 2 * max_rows * ((out_w + 3) // 4) * 12                          # am_image_resample_workspace_bytes
    table = IP.normalisation_table()
    SA, FA, TA, NA = (Input(t, dev) for t in (torch.from_numpy(src), torch.frombuffer(bytearray(bytes(frames)), dtype=torch.uint8),
                                             torch.from_numpy(taps), torch.from_numpy(np.ascontiguousarray(table, np.float32))))

    def call(zero, short=False):
        u8, pix = out_arena((2, out_h, out_w, 3), torch.uint8, dev), out_arena((2, 3, out_h, out_w), torch.float32, dev)
        ws = workspace(need, dev, zero)
        a = L.AmImageResampleArgs()
        a.src, a.src_bytes, a.src_channels, a.fill, a.composite = SA.ptr, src_bytes, 3, 255, None
        a.n_frames, a.out_w, a.out_h = 2, out_w, out_h
        a.frames, a.frames_dev, a.taps, a.taps_dev, a.taps_len = C.addressof(frames), FA.ptr, taps.ctypes.data, TA.ptr, taps.size
        a.norm_table, a.out_pixels, a.out_u8 = NA.ptr, pix.view.data_ptr(), u8.view.data_ptr()
        a.workspace, a.workspace_bytes = ws.view.data_ptr(), need - 1 if short else need
        status = lib.am_image_resample(C.byref(a), stream())
        torch.cuda.synchronize()
        u8.assert_untouched("out_u8"), pix.assert_untouched("out_pixels"), ws.assert_untouched("workspace")
        for i, what in ((SA, "src"), (FA, "frames_dev"), (TA, "taps_dev"), (NA, "norm_table")):
            i.unchanged(what)
        if short:
            refused(lib, status, need)
            assert (ws.view == 0xA5).all() and (u8.view == 0xA5).all(), "something was launched"
            return None
        assert status == 0, lib.am_last_error()
        return {"u8": u8.view.clone(), "pixels": pix.view.clone()}

    got = {k: t.cpu().numpy() for k, t in both_fills(call).items()}
    want = np.stack([np.asarray(Image.fromarray(_padded(im, s)).resize((out_w, out_h), Image.BICUBIC)) for im, s in zip(img, sources)])
    assert int((got["u8"] != want).sum()) == 0
    want_pix = np.stack([table[c][want[..., c]] for c in range(3)], axis=1)
    assert np.array_equal(got["pixels"].view(np.uint32), want_pix.view(np.uint32))
    call(False, short=True)


@pytest.mark.parametrize("channels", [3, 4], ids=["rgb", "rgba"])
def test_image_materialize_guards(dev, lib, channels):
    """Two frames of 3 x 3 pixels plus padding, 15 pixels = 45 bytes each: no multiple of 12, so the last thread of a frame stores
    byte by byte; the second frame starts at 48, right behind the first rounded to 4, and the three bytes between stay sentinels."""
    rng = np.random.default_rng(channels)
    stored = [rng.integers(0, 256, (5, 4, channels), dtype=np.uint8), rng.integers(0, 256, (3, 3, channels), dtype=np.uint8)]
    off1 = (stored[0].size + 3) // 4 * 4
    src_bytes = off1 + stored[1].size
    src = np.full(src_bytes, 0xA5, np.uint8)
    src[: stored[0].size], src[off1:] = stored[0].reshape(-1), stored[1].reshape(-1)
    sources = [IP._Source(0, 4, 5, 1, 1, 3, 3, 1, 0), IP._Source(off1, 3, 3, 0, 0, 3, 3, 0, 1)]
    nbytes = [(s.w + 2 * s.pad_x) * (s.h + 2 * s.pad_y) * 3 for s in sources]
    assert nbytes == [45, 45] and nbytes[0] % 12 != 0
    dst = [0, (nbytes[0] + 3) // 4 * 4]
    out_bytes = dst[1] + nbytes[1]
    frames = _frame_array(sources, dst)
    comp = IP.composite_table()
    SA, FA = Input(torch.from_numpy(src), dev), Input(torch.frombuffer(bytearray(bytes(frames)), dtype=torch.uint8), dev)
    CA = Input(torch.from_numpy(comp.reshape(-1).copy()), dev) if channels == 4 else None
    out = out_arena((out_bytes,), torch.uint8, dev)
    a = L.AmImageMaterializeArgs()
    a.src, a.src_bytes, a.src_channels, a.fill, a.composite = SA.ptr, src_bytes, channels, 255, (CA.ptr if CA else None)
    a.n_frames, a.frames, a.frames_dev, a.out, a.out_bytes = 2, C.addressof(frames), FA.ptr, out.view.data_ptr(), out_bytes
    assert lib.am_image_materialize(C.byref(a), stream()) == 0, lib.am_last_error()
    torch.cuda.synchronize()
    out.assert_untouched("out")
    SA.unchanged("src"), FA.unchanged("frames_dev")
    if CA:
        CA.unchanged("composite")
    got = out.view.cpu().numpy()
    for i, (im, s) in enumerate(zip(stored, sources)):
        rgb = im[..., :3] if channels == 3 else np.stack([comp[im[..., c], im[..., 3]] for c in range(3)], -1)
        assert np.array_equal(got[dst[i]: dst[i] + nbytes[i]], _padded(rgb, s).reshape(-1)), i
    assert (got[nbytes[0]: dst[1]] == 0xA5).all(), "the gap between the frames was written"
    a.out_bytes = out_bytes - 1                                                    # the last frame no longer fits: refused on the host
    fresh = out_arena((out_bytes,), torch.uint8, dev)
    a.out = fresh.view.data_ptr()
    assert lib.am_image_materialize(C.byref(a), stream()) != 0 and str(out_bytes - 1) in lib.am_last_error().decode()
    torch.cuda.synchronize()
    fresh.assert_untouched("out")
    assert (fresh.view == 0xA5).all(), "something was launched"


@pytest.mark.parametrize("T,H,W", [(2, 37, 53), (1, 16, 16)])
def test_image_alpha_stats_guards(dev, lib, T, H, W):
    rng = np.random.default_rng(H)
    rgba = rng.integers(0, 256, (T, H, W, 4), dtype=np.uint8)
    rgba[..., 3] = np.where(rng.random((T, H, W)) < 0.6, 0, rgba[..., 3])
    rgba[:, :2] = 0
    rgba[:, :, :3] = 0
    rgba[:, -1, -1, 3] = 255                                                      # the very last pixel of every frame counts
    RA = Input(torch.from_numpy(rgba), dev)
    stats = out_arena((T, 8), torch.int32, dev)
    a = L.AmImageAlphaStatsArgs()
    a.rgba, a.n_frames, a.height, a.width, a.out_stats = RA.ptr, T, H, W, stats.view.data_ptr()
    assert lib.am_image_alpha_stats(C.byref(a), stream()) == 0, lib.am_last_error()
    torch.cuda.synchronize()
    stats.assert_untouched("out_stats")
    RA.unchanged("rgba")
    got = stats.view.cpu().numpy()
    for t in range(T):
        al = rgba[t, ..., 3]
        ys, xs = np.nonzero(al > 0)
        assert list(got[t]) == [int((al > 127).sum()), xs.min(), ys.min(), xs.max(), ys.max(), 0, 0, 0], t
