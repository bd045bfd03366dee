"""am_render_normals on the device (INTEGRATION.md seam S6) against an fp64 NumPy restatement of the conventions in
include/actionmesh_amd.h - a brute-force test of every sub-pixel against every face - and against geometry worked out by hand:
an analytic sphere, a marker's side of the image, depth order and ties, edges, clipping, determinism, batching, and the
end-to-end grid file.  Parity with PyTorch3D itself is unpinned: it is not installable offline."""
import os

import numpy as np
import pytest
import torch

from actionmesh_amd import render as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- meshes ---------------------------------------------------------------------------------------------------------------
def icosphere(level: int, radius: float = 1.0):
    t = (1.0 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    verts = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = verts[a] + verts[b]
                verts.append(p / np.linalg.norm(p))
                mid[k] = len(verts) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(verts) * radius, np.array(f, dtype=np.int64)


def octahedron(centre, r):
    v = np.array([(r, 0, 0), (-r, 0, 0), (0, r, 0), (0, -r, 0), (0, 0, r), (0, 0, -r)], dtype=np.float64) + np.asarray(centre)
    f = np.array([(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)], dtype=np.int64)
    return v, f


def cam(Rm=np.eye(3), T=(0.0, 0.0, 2.0), f=1.0):
    return {"R": torch.tensor(np.asarray(Rm), dtype=torch.float32), "T": torch.tensor(T, dtype=torch.float32),
            "focal_length": torch.tensor([f, f]), "principal_point": torch.zeros(2)}


def render(verts, faces, cams, S, **kw):
    v = torch.as_tensor(np.asarray(verts), dtype=torch.float32)
    if v.dim() == 2:
        v = v[None]
    out = R.HipRenderer(S).render_normals(v.to(DEV), torch.as_tensor(faces), cams, return_fragments=True, return_float=True, **kw)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in out.items()}


# ---- fp64 restatement ------------------------------------------------------------------------------------------------------
def vertex_normals(V, F):
    fn = np.cross(V[F[:, 2]] - V[F[:, 1]], V[F[:, 0]] - V[F[:, 1]])
    n = np.zeros_like(V)
    for k in range(3):
        np.add.at(n, F[:, k], fn)
    return n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-6)


def restate(V, F, camd, S, tol=1e-5):
    """Every sub-pixel of the 2S x 2S raster against every face, in fp64, with the three rejections of the header: all depths
    negative, |area| <= 1e-8, centre outside the closed box of the projected vertices.  Returns the face index, the clipped
    barycentrics, a `stable` flag (centre more than `tol` NDC from the boundary of every face that covers or nearly covers it - for a
    face with a vertex behind the camera: from the lines through its edges and from its box - and the two nearest depths more than
    `tol` apart), and the S x S mask / normal / rgba8 of the resolve."""
    W = 2 * S
    Rm, T = camd["R"].double().numpy(), camd["T"].double().numpy()
    f, p = camd["focal_length"].double().numpy(), camd["principal_point"].double().numpy()
    Xv = V @ Rm + T
    P = np.stack([f[0] * Xv[:, 0] / Xv[:, 2] + p[0], f[1] * Xv[:, 1] / Xv[:, 2] + p[1], Xv[:, 2]], 1)
    xs = 1 - (2 * np.arange(W) + 1) / W
    Xa, Ya = np.meshgrid(xs, xs)                   # [row, col]: x from the column, y from the row
    best = np.full((W, W), np.inf); second = np.full((W, W), np.inf)
    face = np.full((W, W), -1); bary = np.full((W, W, 3), -1.0); stable = np.ones((W, W), bool)

    def edge(px, py, a, b):
        return (px - a[0]) * (b[1] - a[1]) - (py - a[1]) * (b[0] - a[0])

    for fi, (i0, i1, i2) in enumerate(F):
        v0, v1, v2 = P[i0], P[i1], P[i2]
        if max(v0[2], v1[2], v2[2]) < 0 or abs(edge(v0[0], v0[1], v1, v2)) <= 1e-8:
            continue
        # no centre outside the closed box of the three projected vertices is covered; the window adds a margin for `stable`
        lo, hi = np.minimum(np.minimum(v0, v1), v2)[:2], np.maximum(np.maximum(v0, v1), v2)[:2]
        cs = np.nonzero((xs >= lo[0] - 4.0 / W) & (xs <= hi[0] + 4.0 / W))[0]
        rs = np.nonzero((xs >= lo[1] - 4.0 / W) & (xs <= hi[1] + 4.0 / W))[0]
        if len(cs) == 0 or len(rs) == 0:
            continue
        win = (slice(rs[0], rs[-1] + 1), slice(cs[0], cs[-1] + 1))
        front = min(v0[2], v1[2], v2[2]) > 0
        X, Y = Xa[win], Ya[win]
        area = edge(v2[0], v2[1], v0, v1)
        w = np.stack([edge(X, Y, v1, v2), edge(X, Y, v2, v0), edge(X, Y, v0, v1)], -1) / area
        t = np.stack([w[..., 0] * v1[2] * v2[2], v0[2] * w[..., 1] * v2[2], v0[2] * v1[2] * w[..., 2]], -1)
        pb = t / np.maximum(t.sum(-1, keepdims=True), 1e-8)
        inside = (pb > 0).all(-1)
        cb = np.maximum(pb, 0)
        cb = cb / np.maximum(cb.sum(-1, keepdims=True), 1e-5)
        z = cb @ np.array([v0[2], v1[2], v2[2]])
        cov = inside & (z >= 0) & (X >= lo[0]) & (X <= hi[0]) & (Y >= lo[1]) & (Y <= hi[1])
        # distance of every centre to the triangle's boundary: its segments for a face in front of the camera; for a face with a
        # vertex behind it the barycentrics change sign on the whole LINES through the edges, and the box decides as well
        d = np.full(X.shape, np.inf)
        for a, b in ((v0, v1), (v1, v2), (v2, v0)):
            ab = b[:2] - a[:2]
            s = ((X - a[0]) * ab[0] + (Y - a[1]) * ab[1]) / max(ab @ ab, 1e-300)
            s = np.clip(s, 0, 1) if front else s
            d = np.minimum(d, np.hypot(X - a[0] - s * ab[0], Y - a[1] - s * ab[1]))
        if not front:
            for k, A in enumerate((X, Y)):
                d = np.minimum(d, np.minimum(np.abs(A - lo[k]), np.abs(A - hi[k])))
        stable[win] &= d > tol
        b_, s_ = best[win], second[win]
        closer = cov & (z < b_)
        second[win] = np.where(cov & ~closer, np.minimum(s_, z), np.where(closer, b_, s_))
        best[win] = np.where(closer, z, b_)
        face[win] = np.where(closer, fi, face[win])
        bary[win] = np.where(closer[..., None], cb, bary[win])
    with np.errstate(invalid="ignore"):
        stable &= ~(np.isfinite(second) & (second - best <= tol))
    vn = vertex_normals(V, F)
    cov = face >= 0
    n = np.where(cov[..., None], np.einsum("hwk,hwkc->hwc", np.where(cov[..., None], bary, 0), vn[F[np.maximum(face, 0)]]), 0.0)
    mask = cov.reshape(S, 2, S, 2).sum((1, 3)) / 4.0
    m = n[::2, ::2] @ Rm + T / 2
    u = np.clip((m / np.maximum(np.linalg.norm(m, axis=-1, keepdims=True), 1e-12) + 1) / 2, 0, 1)
    rgb = u * mask[..., None] + (1 - mask[..., None])
    rgba = np.concatenate([rgb, mask[..., None]], -1)
    return dict(face=face, bary=bary, stable=stable, mask=mask, normal=u, rgba8=np.floor(rgba * 255).astype(np.int64))


def check_against_restatement(V, F, cams, S, got=None):
    got = render(V, F, cams, S) if got is None else got
    compared = 0
    for c, camd in enumerate(cams):
        ref = restate(V, F, camd, S)
        st = ref["stable"]
        assert st.mean() > 0.9, st.mean()
        assert np.array_equal(got["pix_to_face"][0, c][st], ref["face"][st]), f"camera {c}: face index differs on stable sub-pixels"
        covered = st & (ref["face"] >= 0)
        assert np.abs(got["bary"][0, c][covered] - ref["bary"][covered]).max() < 1e-4
        px = st.reshape(S, 2, S, 2).all((1, 3))                 # all four sub-pixels stable
        assert np.array_equal(got["mask"][0, c][px], ref["mask"][px])
        assert np.abs(got["normal"][0, c][px] - ref["normal"][px]).max() < 1e-4
        assert np.abs(got["rgba"][0, c][px].astype(np.int64) - ref["rgba8"][px]).max() <= 1
        assert (ref["face"] >= 0).sum() > 100, "the view must show the mesh"
        compared += int(px.sum())
    return compared


def test_jittered_low_poly_matches_restatement():
    V, F = icosphere(2, 0.9)                                              # 320 faces
    rng = np.random.default_rng(3)
    V = V * rng.uniform(0.8, 1.15, size=(len(V), 1)) + rng.normal(0, 0.03, size=V.shape)
    cams = [R.uniform_cameras(distance=3.0)[t] for t in R.VISUALIZER_CAMERAS]
    assert check_against_restatement(V, F, cams, 64) > 3 * 64 * 64 * 0.8


def test_icosphere_matches_restatement():
    V, F = icosphere(3, 0.8)
    V = V + np.array([0.1, -0.05, 0.07])
    cams = [R.uniform_cameras(distance=3.0)[t] for t in R.VISUALIZER_CAMERAS]
    assert check_against_restatement(V, F, cams, 128) > 3 * 128 * 128 * 0.8


def sparse_icosphere():
    """A jittered level-4 icosphere whose 2562 vertices are scattered by a permutation over 3072 rows; the other 510 rows hold
    random positions and are on no face."""
    V0, F0 = icosphere(4, 0.8)
    rng = np.random.default_rng(7)
    V0 = V0 * rng.uniform(0.9, 1.1, size=(len(V0), 1))
    n = 3072
    assert len(V0) == 2562
    rows = rng.permutation(n)[: len(V0)]
    V = rng.normal(0, 0.3, size=(n, 3))
    V[rows] = V0
    return V, rows[F0]


def test_unused_vertices_never_show_and_face_lists_hold_over_the_index_range():
    """The sparse mesh above: used and unused rows interleaved over the whole index range.  A vertex that got the face list of
    another one would have a moved normal; the unused rows' positions and normals must never show."""
    V, F = sparse_icosphere()
    valence = np.bincount(F.reshape(-1), minlength=len(V))
    assert (valence == 0).sum() == len(V) - 2562
    cams = [R.uniform_cameras(distance=3.0)[t] for t in R.VISUALIZER_CAMERAS]
    got = render(V, F, cams, 48)
    assert check_against_restatement(V, F, cams, 48, got) > 3 * 48 * 48 * 0.8
    pf = got["pix_to_face"]
    assert pf.min() == -1 and pf.max() < len(F) and (pf >= 0).sum() > 3 * 2000       # only real faces are named


def test_analytic_sphere():
    S, r, d = 256, 0.8, 3.0
    V, F = icosphere(4, r)
    camd = R.uniform_cameras(distance=d)["U000"]
    got = render(V, F, [camd], S)
    f = 2.1875
    rho = f * r / np.sqrt(d * d - r * r)
    area = got["mask"][0, 0].sum() * (2.0 / S) ** 2
    assert abs(area / (np.pi * rho ** 2) - 1) < 0.01, (area, np.pi * rho ** 2)
    # analytic ray-sphere normal at the centre of sub-pixel (2i, 2j), put through n @ R + T / 2
    Rm, T = camd["R"].double().numpy(), camd["T"].double().numpy()
    W = 2 * S
    xs = 1 - (2 * np.arange(0, W, 2) + 1) / W
    X, Y = np.meshgrid(xs, xs)
    dirs = np.stack([X / f, Y / f, np.ones_like(X)], -1) @ Rm.T
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    o = -T @ Rm.T
    b = dirs @ o
    disc = b * b - (o @ o - r * r)
    full = (got["mask"][0, 0] == 1.0) & (disc > 0)
    tt = -b - np.sqrt(np.maximum(disc, 0))
    n = (o + tt[..., None] * dirs) / r
    m = n @ Rm + T / 2
    m /= np.linalg.norm(m, axis=-1, keepdims=True)
    g = 2 * got["normal"][0, 0].astype(np.float64) - 1
    g /= np.linalg.norm(g, axis=-1, keepdims=True)
    ang = np.degrees(np.arccos(np.clip((g * m).sum(-1), -1, 1)))[full]
    assert full.sum() > 0.9 * np.pi * (rho * S / 2) ** 2
    assert ang.mean() < 1.0 and ang.max() < 3.0, (ang.mean(), ang.max())


def test_marker_lands_where_the_hand_derived_convention_puts_it():
    """U000 looks along -X (world +Z is view +x), U004 along +Z (world +X is view +x), U008 along +X (world -Z is view +x); NDC +x
    is the LEFT of the image and +y the top.  A marker at (0.5, 0.5, 0.5) is therefore upper-left, upper-left, upper-right."""
    V, F = octahedron((0.5, 0.5, 0.5), 0.1)
    cams = R.uniform_cameras(distance=3.0)
    S = 64
    got = render(V, F, [cams[t] for t in R.VISUALIZER_CAMERAS], S)
    for c, side in enumerate(("left", "left", "right")):
        m = got["mask"][0, c]
        assert m.sum() > 4
        rows, cols = np.nonzero(m)
        assert rows.mean() < S / 2 - 4, (c, rows.mean())
        assert (cols.mean() < S / 2 - 4) if side == "left" else (cols.mean() > S / 2 + 4), (c, cols.mean())


def test_depth_order_and_ties():
    # two overlapping triangles facing the camera (view = X + (0, 0, 2)): the one at z = 0 is nearer than the one at z = 0.5
    near = [(-0.5, -0.5, 0.0), (0.6, -0.4, 0.0), (0.0, 0.6, 0.0)]
    far = [(-1.0, -1.0, 0.5), (1.2, -0.8, 0.5), (-0.2, 1.2, 0.5)]
    alone = render(np.array(near), np.array([[0, 1, 2]]), [cam()], 32)["pix_to_face"][0, 0] >= 0
    assert alone.sum() > 100
    for order in ((near, far), (far, near)):
        V = np.array(order[0] + order[1])
        F = np.array([[0, 1, 2], [3, 4, 5]])
        got = render(V, F, [cam()], 32)
        pf = got["pix_to_face"][0, 0]
        nearest = 0 if order[0] is near else 1
        assert (pf[alone] == nearest).all(), "the nearer triangle must win wherever it covers"
        assert (pf[~alone & (pf >= 0)] == 1 - nearest).all() and (pf == 1 - nearest).sum() > 100   # the far one shows around it
    # two faces on the same three vertices: the lower index wins, with either winding order of the same triplet repeated
    V = np.array(near)
    got = render(V, np.array([[0, 1, 2], [0, 1, 2]]), [cam()], 32)
    pf = got["pix_to_face"][0, 0]
    assert (pf >= 0).sum() > 100 and (pf[pf >= 0] == 0).all()
    got = render(V, np.array([[2, 1, 0], [2, 1, 0], [2, 1, 0]]), [cam()], 32)
    pf = got["pix_to_face"][0, 0]
    assert (pf >= 0).sum() > 100 and (pf[pf >= 0] == 0).all()


def test_frame_filling_quad_behind_camera_and_half_plane():
    S = 64
    # view = X + (0, 0, 2), f = 1: the quad reaches NDC +-1.5; its diagonal y = x - 0.05 (NDC y = x - 0.025) misses every centre
    V = np.array([(-3.0, -3.05, 0.0), (3.0, -3.05, 0.0), (3.0, 2.95, 0.0), (-3.0, 2.95, 0.0)])
    F = np.array([[0, 1, 2], [0, 2, 3]])
    got = render(V, F, [cam()], S)
    assert (got["pix_to_face"] >= 0).all() and (got["mask"] == 1.0).all() and (got["rgba"][..., 3] == 255).all()
    assert set(np.unique(got["pix_to_face"])) == {0, 1}
    # the same quad behind the camera
    got = render(V, F, [cam(T=(0.0, 0.0, -2.0))], S)
    assert (got["mask"] == 0).all() and (got["pix_to_face"] == -1).all()
    assert (got["rgba"][..., :3] == 255).all() and (got["rgba"][..., 3] == 0).all()
    # a half plane with a slanted edge: partial coverage only in quarters
    V = np.array([(-5.0, -5.0, 0.0), (0.3, -5.0, 0.0), (-0.2, 5.0, 0.0)])
    got = render(V, np.array([[0, 1, 2]]), [cam()], S)
    vals = set(np.unique(got["mask"]).tolist())
    assert vals <= {0.0, 0.25, 0.5, 0.75, 1.0} and {0.0, 1.0} <= vals and len(vals) > 2
    assert set(np.unique(got["rgba"][..., 3]).tolist()) <= {0, 63, 127, 191, 255}


def test_faces_straddling_the_camera_plane():
    """A face with a vertex behind the camera has barycentrics > 0 in the cone beyond the vertex on the other side of the camera
    plane.  For the two triangles here that vertex's projection is extreme in y, so the whole cone lies OUTSIDE the box of the
    projected vertices, and the box rule of include/actionmesh_amd.h skips every centre outside the box: these faces cover nothing,
    whatever the resolution.  (Not every such face: where that vertex projects extreme on neither axis, part of the cone lies inside
    the box and stays covered.)  pix_to_face is compared with the restatement on every sub-pixel more than 1e-5 from a box edge or
    an edge's line (restate() counts both for such a face), not on a subset chosen by hand."""
    two_behind = np.array([(-0.5, -0.5, -3.0), (0.6, -0.4, -3.0), (0.0, 0.3, 0.0)])      # view z = -1, -1, 2 with cam()
    one_behind = np.array([(-0.5, -0.5, 0.0), (0.6, -0.4, 0.0), (0.0, 0.3, -3.0)])       # view z = 2, 2, -1
    tri = np.array([[0, 1, 2]])
    for S in (32, 45):
        for V in (two_behind, one_behind):
            got = render(V, tri, [cam()], S)
            ref = restate(V, tri, cam(), S)
            assert (ref["face"] == -1).all() and ref["stable"].mean() > 0.9
            st = ref["stable"]
            assert np.array_equal(got["pix_to_face"][0, 0][st], ref["face"][st])
            assert (got["pix_to_face"] == -1).all() and (got["bary"] == -1).all(), int((got["pix_to_face"] >= 0).sum())
            assert (got["mask"] == 0).all() and (got["rgba"][..., :3] == 255).all() and (got["rgba"][..., 3] == 0).all()
    # the first triangle in front of a frame-filling quad (the one of the test below, at view z = 2.5): the quad shows everywhere
    S = 32
    quad = np.array([(-3.0, -3.05, 0.5), (3.0, -3.05, 0.5), (3.0, 2.95, 0.5), (-3.0, 2.95, 0.5)])
    V = np.concatenate([quad, two_behind])
    F = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6]])
    got = render(V, F, [cam()], S)
    ref = restate(V, F, cam(), S)
    st = ref["stable"]
    assert st.mean() > 0.9 and set(np.unique(ref["face"])) == {0, 1}
    assert np.array_equal(got["pix_to_face"][0, 0][st], ref["face"][st])
    assert set(np.unique(got["pix_to_face"])) == {0, 1} and (got["mask"] == 1.0).all() and (got["rgba"][..., 3] == 255).all()


def test_deterministic_and_batch_independent():
    V0, F = icosphere(3, 0.7)
    T = 3
    Vt = np.stack([V0 * (1 + 0.1 * t) + np.array([0.05 * t, 0.0, -0.03 * t]) for t in range(T)])
    cams = [R.uniform_cameras(distance=3.0)[t] for t in R.VISUALIZER_CAMERAS]
    a = render(Vt, F, cams, 96)
    b = render(Vt, F, cams, 96)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    for t in range(T):
        for c in range(len(cams)):
            s = render(Vt[t], F, [cams[c]], 96)
            for k in a:
                assert np.array_equal(a[k][t, c].view(np.uint8), s[k][0, 0].view(np.uint8)), (k, t, c)


def test_face_index_outside_the_mesh_is_a_value_error():
    """The faces are validated on the device: one index equal to V is reported behind the launch, in the mesh stage's words."""
    from actionmesh_amd import ops
    V, F = octahedron((0.0, 0.0, 0.0), 0.5)
    verts = torch.as_tensor(V, dtype=torch.float32)[None].to(DEV)
    clean = ops.render_normals(verts, torch.as_tensor(F), [cam()], 8)
    assert int(clean["rgba"][..., 3].max()) > 0
    bad = F.copy()
    bad[5, 1] = len(V)
    with pytest.raises(ValueError, match=r"a face names a vertex outside \[0, 6\)"):
        ops.render_normals(verts, torch.as_tensor(bad), [cam()], 8)


def test_visualizer_end_to_end(tmp_path):
    from PIL import Image
    V0, F = icosphere(3, 0.6)
    T = 16
    Vt = np.stack([V0 * np.array([1 + 0.02 * t, 1.0, 1 - 0.01 * t]) + np.array([0.0, 0.02 * t, 0.0]) for t in range(T)])

    class Mesh:
        def __init__(self, v):
            self.vertices, self.faces = v, F
    meshes = [Mesh(v) for v in Vt]
    rng = np.random.default_rng(0)
    frames = [Image.fromarray(rng.integers(0, 256, size=(120, 90, 3), dtype=np.uint8), "RGB") for _ in range(T)]
    vis = R.HipVisualizer(image_size=256)
    paths, grid = vis.render(meshes, device=DEV, output_dir=str(tmp_path / "out"), input_frames=frames)
    assert len(paths) == 1 and os.path.basename(paths[0]).startswith("grid_normal.") and os.path.isfile(paths[0])
    assert len(grid) == T and all(g.size == (1024, 256) for g in grid)
    expect = R.resample_list(frames, T)
    for t in range(T):
        assert np.array_equal(np.array(grid[t])[:, :256, :3], np.array(expect[t].resize((256, 256))))
    if paths[0].endswith(".png"):
        im = Image.open(paths[0])
        assert im.n_frames == T and im.size == (1024, 256)
        im.seek(5)
        assert np.array_equal(np.array(im.convert("RGB")), np.array(grid[5].convert("RGB")))
    # the (T, V, 3) stack with faces= gives the same frames
    _, grid2 = vis.render(Vt, device=DEV, output_dir=str(tmp_path / "out2"), input_frames=frames, faces=F)
    assert all(np.array_equal(np.array(a), np.array(b)) for a, b in zip(grid, grid2))
    # the normal columns show the sphere on white
    col = np.array(grid[0])[:, 256:512]
    assert (col[0, 0, :3] == 255).all() and col[0, 0, 3] == 0
    assert col[128, 128, 3] == 255 and not (col[128, 128, :3] == 255).all()
