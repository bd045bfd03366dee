"""What the mesh-decimation tests share: the test meshes, a numpy fp64 restatement of the four kernels of csrc/am_decimate.hip written
from the text of include/actionmesh_amd.h (every product, sum and quotient its own numpy call, in the header's order, so the device
is compared bit for bit), wrapped as the backend object `mesh_decimate.decimate_mesh` takes, the mesh invariants, and a sequential
greedy quadric decimation (a heap, one collapse at a time, the same cost and validity rules) as the quality yardstick."""
import heapq

import numpy as np
import torch

NO_KEY = np.int64(2 ** 63 - 1)
ZERO, COND, REACH, FLIP = 1e-13, 1e-10, 4.0, 0.2
BAD_FACE, BAD_CSR, BAD_EDGE, BAD_KEPT = 1, 2, 4, 8


# ---- meshes -----------------------------------------------------------------------------------------------------------------------------
def icosphere(level):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        cache, g = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                cache[k] = len(v) - 1
            return cache[k]

        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return np.array(v), np.array(f, dtype=np.int64)


def torus(nu, nv, R=1.0, r=0.4):
    a, b = np.meshgrid(np.arange(nu) * (2 * np.pi / nu), np.arange(nv) * (2 * np.pi / nv), indexing="ij")
    v = np.stack(((R + r * np.cos(b)) * np.cos(a), (R + r * np.cos(b)) * np.sin(a), r * np.sin(b)), -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    p00, p10 = i * nv + j, (i + 1) % nu * nv + j
    p01, p11 = i * nv + (j + 1) % nv, (i + 1) % nu * nv + (j + 1) % nv
    f = np.concatenate((np.stack((p00, p10, p11), -1).reshape(-1, 3), np.stack((p00, p11, p01), -1).reshape(-1, 3)))
    return v, f.astype(np.int64)


def jittered_icosphere(level, scale=0.004, seed=5):
    v, f = icosphere(level)
    return v + np.random.default_rng(seed).normal(scale=scale, size=v.shape), f


def grid(n):
    """A flat open n x n grid of vertices in the plane z = 0."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack((i, j, np.zeros_like(i)), -1).reshape(-1, 3).astype(np.float64)
    a = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
    f = np.concatenate((np.stack((a, a + n, a + n + 1), -1), np.stack((a, a + n + 1, a + 1), -1)))
    return v, f.astype(np.int64)


def tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64)
    return v, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], dtype=np.int64)


def glued_tetrahedra():
    """Two tetrahedra glued along a face: a closed surface of 5 vertices and 6 faces in which every edge fails the link condition."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.3, 0.3, 1], [0.3, 0.3, -1]], dtype=np.float64)
    return v, np.array([[0, 1, 3], [1, 2, 3], [2, 0, 3], [1, 0, 4], [2, 1, 4], [0, 2, 4]], dtype=np.int64)


def hub(n=40):
    """A closed bipyramid: two vertices of valence n over a ring of n vertices of valence 4."""
    a = np.arange(n) * (2 * np.pi / n)
    v = np.concatenate((np.stack((np.cos(a), np.sin(a), 0.05 * np.cos(3 * a)), -1), [[0, 0, 0.7], [0, 0, -0.7]]))
    i = np.arange(n)
    j = (i + 1) % n
    f = np.concatenate((np.stack((i, j, np.full(n, n)), -1), np.stack((j, i, np.full(n, n + 1)), -1)))
    return v, f.astype(np.int64)


def finned_sphere():
    """An icosphere with one more face on one of its edges: that edge is shared by three faces.  Returns (v, f, (a, b))."""
    v, f = icosphere(2)
    a, b = int(f[7, 0]), int(f[7, 1])
    w = (v[a] + v[b]) * 0.8
    return np.concatenate((v, w[None])), np.concatenate((f, [[a, b, len(v)]])), (a, b)


# ---- numpy tables -----------------------------------------------------------------------------------------------------------------------
def np_topology(faces, V):
    flat = faces.reshape(-1)
    order = np.argsort(flat, kind="stable")
    offsets = np.searchsorted(flat[order], np.arange(V + 1))
    return offsets.astype(np.int32), order.astype(np.int32)


def np_edges(faces, V):
    f = faces.astype(np.int64)
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    uniq, inverse, counts = np.unique(np.minimum(a, b) * V + np.maximum(a, b), return_inverse=True, return_counts=True)
    return np.stack((uniq // V, uniq % V), 1).astype(np.int32), inverse.reshape(-1).astype(np.int32), counts.astype(np.int32)


def validate(V, faces, offsets, corners, edges=None, he2e=None, kept=None):
    """The flag bits of inconsistent tables.  The device flags only what a thread meets; these are the same conditions on everything."""
    bits, F = 0, faces.shape[0]
    if ((faces < 0) | (faces >= V)).any():
        bits |= BAD_FACE
    o = offsets.astype(np.int64)
    if (o < 0).any() or (np.diff(o) < 0).any() or (o > 3 * F).any():
        bits |= BAD_CSR
    else:
        c = corners.astype(np.int64)[o[0]:o[-1]]
        owner = np.repeat(np.arange(V), np.diff(o))
        inside = (c >= 0) & (c < 3 * F)
        if not inside.all() or (faces.reshape(-1)[c] != owner).any():
            bits |= BAD_CSR
    if edges is not None:
        if ((edges < 0) | (edges >= V)).any() or (edges[:, 0] > edges[:, 1]).any():
            bits |= BAD_EDGE
        if he2e is not None and not bits & BAD_FACE:
            if ((he2e < 0) | (he2e >= edges.shape[0])).any():
                bits |= BAD_EDGE
            else:
                a, b = faces.reshape(-1), faces[:, [1, 2, 0]].reshape(-1)
                if (edges[he2e, 0] != np.minimum(a, b)).any() or (edges[he2e, 1] != np.maximum(a, b)).any():
                    bits |= BAD_EDGE
    if kept is not None and ((kept < 0) | (kept >= edges.shape[0])).any():
        bits |= BAD_KEPT
    return bits


# ---- the header's arithmetic ------------------------------------------------------------------------------------------------------------
def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack((a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]), -1)


def mix32(h):
    h = h.astype(np.uint64)
    m = np.uint64(0xffffffff)
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85ebca6b)) & m
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xc2b2ae35)) & m
    return h ^ (h >> np.uint64(16))


def quadric_cost(q, y):
    r = [((q[:, i0] * y[:, 0] + q[:, i1] * y[:, 1]) + q[:, i2] * y[:, 2]) + q[:, i3]
         for i0, i1, i2, i3 in ((0, 1, 2, 3), (1, 4, 5, 6), (2, 5, 7, 8), (3, 6, 8, 9))]
    return ((r[0] * y[:, 0] + r[1] * y[:, 1]) + r[2] * y[:, 2]) + r[3]


def _expand(offsets, corners, faces, s):
    """Every corner of the vertices `s` (one row per corner, in CSR order): (row -> position in s, corner id, face, k, w1, w2)."""
    o = offsets.astype(np.int64)
    n = o[s + 1] - o[s]
    rep = np.repeat(np.arange(s.shape[0]), n)
    within = np.arange(rep.shape[0]) - np.repeat(np.cumsum(n) - n, n)
    c = corners[o[s][rep] + within].astype(np.int64)
    f, k = c // 3, c % 3
    return rep, c, f, k, faces[f, (k + 1) % 3].astype(np.int64), faces[f, (k + 2) % 3].astype(np.int64)


def ref_quadrics(pos, faces, offsets, corners):
    V = pos.shape[0]
    p0, p1, p2 = pos[faces[:, 0]], pos[faces[:, 1]], pos[faces[:, 2]]
    c = cross(p1 - p0, p2 - p0)
    length = np.sqrt(dot(c, c))
    good = length > ZERO
    with np.errstate(invalid="ignore", divide="ignore"):
        n = c / length[:, None]
        d = -dot(n, p0)
        w = length / 2.0
        p = np.concatenate((n, d[:, None]), 1)
        qf = np.stack([(w * p[:, a]) * p[:, b] for a in range(4) for b in range(a, 4)], 1)
    qf = np.where(good[:, None], qf, 0.0)
    o = offsets.astype(np.int64)
    valence = np.diff(o)
    Q = np.zeros((V, 10))
    for j in range(int(valence.max())):
        vs = np.nonzero(valence > j)[0]
        Q[vs] = Q[vs] + qf[corners[o[vs] + j] // 3]
    return Q


def ref_edges(pos, Q, faces, offsets, corners, edges, he2e, count, subset=None):
    V, E = pos.shape[0], edges.shape[0]
    u, v = edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64)
    cand, cost, key = np.zeros((E, 3)), np.zeros(E), np.full(E, NO_KEY, dtype=np.int64)
    locked = np.zeros(V, dtype=bool)
    locked[edges[count != 2].reshape(-1)] = True
    valence = np.diff(offsets.astype(np.int64))
    ok = (u < v) & (count == 2) & ~locked[u] & ~locked[v]
    if subset is not None:
        only = np.zeros(E, dtype=bool)
        only[subset] = True
        ok &= only
    idx = np.nonzero(ok)[0]
    if idx.size == 0:
        return cand, cost, key
    ekey = u * V + v
    if not (np.diff(ekey) > 0).all():
        ekey = np.unique(ekey)
    ui, vi = u[idx], v[idx]
    # link: the apexes, and the neighbours of u that are neighbours of v
    rep, _, _, _, w1, w2 = _expand(offsets, corners, faces, ui)
    o = vi[rep]
    has = (w1 == o) | (w2 == o)
    n_apex = np.bincount(rep, weights=has, minlength=idx.size).astype(np.int64)

    def adj(w):                                                                # is { w, o } an edge?
        k = np.minimum(w, o) * V + np.maximum(w, o)
        return (w != o) & (ekey[np.minimum(np.searchsorted(ekey, k), ekey.shape[0] - 1)] == k)

    shared = np.bincount(rep, weights=adj(w1).astype(np.int64) + adj(w2), minlength=idx.size).astype(np.int64)
    rows = np.nonzero(has & (n_apex[rep] == 2))[0]
    a0, a1 = np.full(idx.size, -1, dtype=np.int64), np.full(idx.size, -1, dtype=np.int64)
    apex = np.where(w1 == o, w2, w1)
    a0[rep[rows[0::2]]] = apex[rows[0::2]]
    a1[rep[rows[1::2]]] = apex[rows[1::2]]
    link = (n_apex == 2) & (shared == 4) & (a0 != a1) & (a0 != ui) & (a0 != vi) & (a1 != ui) & (a1 != vi)
    link &= (valence[np.maximum(a0, 0)] > 3) & (valence[np.maximum(a1, 0)] > 3)
    idx, ui, vi, a0, a1 = idx[link], ui[link], vi[link], a0[link], a1[link]
    if idx.size == 0:
        return cand, cost, key
    # position and cost
    q = Q[ui] + Q[vi]
    pu, pv = pos[ui], pos[vi]
    mid = (pu + pv) * 0.5
    edge = pv - pu
    a, b, c, d, e, f = q[:, 0], q[:, 1], q[:, 2], q[:, 4], q[:, 5], q[:, 7]
    r0, r1, r2 = -q[:, 3], -q[:, 6], -q[:, 8]
    m0, m1, m2 = d * f - e * e, b * f - e * c, b * e - d * c
    det = (a * m0 - b * m1) + c * m2
    s, t, g = r1 * f - e * r2, r1 * e - d * r2, b * r2 - r1 * c
    dx = (r0 * m0 - b * s) + c * t
    dy = (a * s - r0 * m1) + c * g
    dz = (a * (d * r2 - r1 * e) - b * g) + r0 * m2
    tr = (a + d) + f
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        y = np.stack((dx / det, dy / det, dz / det), 1)
        off = y - mid
        solved = (np.abs(det) > COND * ((tr * tr) * tr)) & (dot(off, off) <= REACH * dot(edge, edge))
        cy = quadric_cost(q, y)
    cu, cv, cm = quadric_cost(q, pu), quadric_cost(q, pv), quadric_cost(q, mid)
    x, cx = pu.copy(), cu.copy()
    better = cv < cx
    x[better], cx[better] = pv[better], cv[better]
    better = cm < cx
    x[better], cx[better] = mid[better], cm[better]
    x[solved], cx[solved] = y[solved], cy[solved]
    cx = np.where(cx > 0.0, cx, 0.0)
    cand[idx], cost[idx] = x, cx
    # no flip, and no other face on both apexes
    good = np.ones(idx.size, dtype=bool)
    for s_, o_ in ((ui, vi), (vi, ui)):
        rep, _, fc, k, w1, w2 = _expand(offsets, corners, faces, s_)
        o = o_[rep]
        other = ~((w1 == o) | (w2 == o))
        both = other & (((w1 == a0[rep]) & (w2 == a1[rep])) | ((w1 == a1[rep]) & (w2 == a0[rep])))
        p = pos[faces[fc]]                                                     # (rows, 3 vertices, 3)
        c0 = cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        p[np.arange(rep.shape[0]), k] = x[rep]
        c1 = cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        fine = dot(c0, c1) > (FLIP * np.sqrt(dot(c0, c0))) * np.sqrt(dot(c1, c1))
        bad = both | (other & ~fine)
        good &= np.bincount(rep, weights=bad, minlength=idx.size) == 0
    bits = cx.astype(np.float32).view(np.uint32).astype(np.uint64)
    k64 = ((bits << np.uint64(32)) | mix32(idx)).astype(np.int64)
    key[idx[good]] = k64[good]
    return cand, cost, key


def ref_select(V, edges, key):
    u, v = edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64)
    m1 = np.full(V, NO_KEY, dtype=np.int64)
    np.minimum.at(m1, u, key)
    np.minimum.at(m1, v, key)
    m2 = m1.copy()
    np.minimum.at(m2, u, m1[v])
    np.minimum.at(m2, v, m1[u])
    return m1, m2, ((key != NO_KEY) & (key == m2[u]) & (key == m2[v])).astype(np.uint8)


def ref_apply(pos, Q, faces, offsets, corners, edges, cand, kept, vmap):
    """In place on pos, Q, faces, vmap; returns the dead-face flags."""
    kept = kept.astype(np.int64)
    u, v = edges[kept, 0].astype(np.int64), edges[kept, 1].astype(np.int64)
    pos[u] = cand[kept]
    Q[u] = Q[u] + Q[v]
    rep, c, f, _, w1, w2 = _expand(offsets, corners, faces, v)
    has = (w1 == u[rep]) | (w2 == u[rep])
    dead = np.zeros(faces.shape[0], dtype=np.uint8)
    dead[f[has]] = 1
    faces.reshape(-1)[c[~has]] = u[rep][~has]
    vmap[v] = u
    return dead


class NumpyBackend:
    """The restatement as the backend of mesh_decimate.decimate_rounds, on CPU tensors (which share their memory with numpy)."""

    @staticmethod
    def _flag(flag, bits, V):
        if flag is not None:
            flag[0] = bits
        elif bits:
            from actionmesh_amd import ops
            raise ValueError("decimate (numpy): " + ops.decimate_flag_message(bits, V))
        return bits

    def quadrics(self, positions, faces, topology, flag=None):
        V = positions.shape[0]
        f, o, c = faces.numpy(), topology.offsets.numpy(), topology.corners.numpy()
        if self._flag(flag, validate(V, f, o, c), V):
            return torch.zeros((V, 10), dtype=torch.float64)
        return torch.from_numpy(ref_quadrics(positions.numpy(), f, o, c))

    def edges(self, positions, quadrics, faces, topology, edges, half_edge_to_edge, edge_count, flag=None):
        V, E = positions.shape[0], edges.shape[0]
        f, o, c = faces.numpy(), topology.offsets.numpy(), topology.corners.numpy()
        if self._flag(flag, validate(V, f, o, c, edges.numpy(), half_edge_to_edge.numpy()), V):
            return torch.zeros((E, 3), dtype=torch.float64), torch.zeros(E, dtype=torch.float64), torch.full((E,), int(NO_KEY))
        out = ref_edges(positions.numpy(), quadrics.numpy(), f, o, c, edges.numpy(), half_edge_to_edge.numpy(), edge_count.numpy())
        return tuple(torch.from_numpy(t) for t in out)

    def select(self, n_vertices, faces, topology, edges, half_edge_to_edge, keys, flag=None):
        self._flag(flag, 0, n_vertices)
        return tuple(torch.from_numpy(t) for t in ref_select(n_vertices, edges.numpy(), keys.numpy()))

    def apply(self, positions, quadrics, faces, topology, edges, candidates, kept, vertex_map, flag=None):
        V = positions.shape[0]
        f, o, c = faces.numpy(), topology.offsets.numpy(), topology.corners.numpy()
        if self._flag(flag, validate(V, f, o, c, edges.numpy(), None, kept.numpy()), V):
            return torch.zeros(f.shape[0], dtype=torch.uint8)
        return torch.from_numpy(ref_apply(positions.numpy(), quadrics.numpy(), f, o, c, edges.numpy(), candidates.numpy(), kept.numpy(),
                                          vertex_map.numpy()))


# ---- invariants -------------------------------------------------------------------------------------------------------------------------
def edge_use(faces):
    f = np.sort(np.stack((faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]), 1).reshape(-1, 2), 1)
    return np.unique(f, axis=0, return_counts=True)


def euler(V, faces):
    return V - edge_use(faces)[0].shape[0] + faces.shape[0]


def face_areas(v, f):
    c = cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return np.sqrt(dot(c, c)) / 2.0


def check_closed_manifold(v, f, chi):
    """Every edge in exactly two faces, the Euler characteristic, no repeated index, no duplicate face, positive areas, no
    unreferenced vertex."""
    assert (edge_use(f)[1] == 2).all()
    assert euler(v.shape[0], f) == chi
    assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 2] != f[:, 0]).all()
    assert np.unique(np.sort(f, 1), axis=0).shape[0] == f.shape[0]
    assert (face_areas(v, f) > 0).all()
    assert np.array_equal(np.unique(f), np.arange(v.shape[0]))


def sample_surface(v, f, n, seed):
    rng = np.random.default_rng(seed)
    cdf = np.cumsum(face_areas(v, f))
    face = np.searchsorted(cdf, rng.random(n) * cdf[-1])
    r = rng.random((n, 2))
    fold = r.sum(1) > 1
    r[fold] = 1 - r[fold]
    p0, p1, p2 = v[f[face, 0]], v[f[face, 1]], v[f[face, 2]]
    return p0 + (p1 - p0) * r[:, :1] + (p2 - p0) * r[:, 1:]


def surface_distance(v0, f0, v1, f1, n=20000):
    """The symmetric mean nearest-neighbour distance between n area-uniform samples of each surface (fixed seeds)."""
    from scipy.spatial import cKDTree
    a, b = sample_surface(v0, f0, n, 11), sample_surface(v1, f1, n, 12)
    return 0.5 * (cKDTree(b).query(a)[0].mean() + cKDTree(a).query(b)[0].mean())


# ---- the sequential yardstick -----------------------------------------------------------------------------------------------------------
def greedy_decimate(v, f, target_faces):
    """Sequential greedy quadric decimation: a heap of (cost, u, v), one collapse at a time - the cheapest edge whose stored cost is
    still its cost -, with the cost, position and validity rules of ref_edges.  After a collapse the edges of the surviving vertex are
    re-evaluated; when the heap runs dry every edge is.  Returns (vertices, faces) compacted."""
    V = v.shape[0]
    pos, faces = v.astype(np.float64).copy(), f.astype(np.int32).copy()
    offsets, corners = np_topology(faces, V)
    Q = ref_quadrics(pos, faces, offsets, corners)
    heap = []

    def tables():
        o, c = np_topology(faces, V)
        return (o, c) + np_edges(faces, V)

    def push(t, subset):
        _, cost, key = ref_edges(pos, Q, faces, *t, subset=subset)
        for e in np.nonzero(key != NO_KEY)[0]:
            heapq.heappush(heap, (float(cost[e]), int(t[2][e, 0]), int(t[2][e, 1])))

    t = tables()
    push(t, None)
    reseeded = False
    while faces.shape[0] > target_faces:
        if not heap:
            if reseeded:
                break
            push(t, None)
            reseeded = True
            continue
        c0, a, b = heapq.heappop(heap)
        ekey = t[2][:, 0].astype(np.int64) * V + t[2][:, 1]
        e = int(np.searchsorted(ekey, a * V + b))
        if e >= ekey.shape[0] or ekey[e] != a * V + b:
            continue
        cand, cost, key = ref_edges(pos, Q, faces, *t, subset=np.array([e]))
        if key[e] == NO_KEY:
            continue
        if float(cost[e]) != c0:
            heapq.heappush(heap, (float(cost[e]), a, b))
            continue
        dead = ref_apply(pos, Q, faces, t[0], t[1], t[2], cand, np.array([e]), np.arange(V))
        faces = faces[dead == 0]
        reseeded = False
        t = tables()
        push(t, np.nonzero((t[2][:, 0] == a) | (t[2][:, 1] == a))[0])
    used = np.unique(faces)
    remap = np.full(V, -1)
    remap[used] = np.arange(used.shape[0])
    return pos[used], remap[faces]
