"""What the border-collapse tests share: open test meshes, a numpy fp64 restatement of am_decimate_border_quadrics and
am_decimate_border_edges written from the text of include/actionmesh_amd.h ("Border collapses"), the backend object that puts it behind
`mesh_decimate.decimate_mesh(..., borders="collapse")`, the open-manifold invariants and a sequential greedy decimation with the same
rules.  The arithmetic follows tests/_decimate_ref.py (every product, sum and quotient its own numpy call, in the header's order).  The
TOPOLOGY is not the kernel's case list: `coned_complex` really adds the imaginary vertex and its faces, and `link_condition` applies the
closed link condition to that complex - common neighbours, common link edges, valences - so the two agree only if the case list
follows from the rule."""
import heapq

import numpy as np
import torch

import _decimate_ref as R
from _decimate_ref import NO_KEY, ZERO, COND, REACH, FLIP, BAD_EDGE

INTERIOR, BORDER, LOCKED = 0, 1, 2


# ---- meshes -----------------------------------------------------------------------------------------------------------------------------
def _compact(v, f):
    used = np.unique(f)
    remap = np.full(v.shape[0], -1, dtype=np.int64)
    remap[used] = np.arange(used.shape[0])
    return v[used], remap[f]


def open_cylinder(nu, nv, r=1.0, h=2.0):
    """nu vertices around, nv rings along the axis: an open tube with two border loops (a little radial jitter, so no solve is singular
    by symmetry alone)."""
    a, t = np.meshgrid(np.arange(nu) * (2 * np.pi / nu), np.arange(nv) * (h / (nv - 1)), indexing="ij")
    rr = r + 0.01 * np.random.default_rng(3).normal(size=a.shape)
    v = np.stack((rr * np.cos(a), rr * np.sin(a), t), -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv - 1), indexing="ij")
    p00, p10 = i * nv + j, (i + 1) % nu * nv + j
    p01, p11 = p00 + 1, p10 + 1
    f = np.concatenate((np.stack((p00, p10, p11), -1).reshape(-1, 3), np.stack((p00, p11, p01), -1).reshape(-1, 3)))
    return v, f.astype(np.int64)


def half_icosphere(level):
    """The faces of `jittered_icosphere(level)` whose centroid has z > 0: a cap with one jagged border loop."""
    v, f = R.jittered_icosphere(level)
    return _compact(v, f[v[f].mean(1)[:, 2] > 0])


def holes_grid(n=7):
    """grid(n) without one triangle (a hole of three edges) and without the two triangles of one cell (a hole of four)."""
    v, f = R.grid(n)
    cells = (n - 1) ** 2
    tri, sq = 1 * (n - 1) + 1, (n - 3) * (n - 1) + (n - 3)                    # cell (1, 1) and cell (n - 3, n - 3)
    keep = np.ones(f.shape[0], dtype=bool)
    keep[[tri, sq, cells + sq]] = False
    return v, f[keep]


def isolated_triangle():
    return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float64), np.array([[0, 1, 2]], dtype=np.int64)


def strip():
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], dtype=np.float64)
    return v, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int64)


def ear_disc(n=4):
    """grid(n) with one more triangle on its border edge (0, 1): the new vertex is an ear.  Returns (v, f, index of the ear)."""
    v, f = R.grid(n)
    ear = np.array([[-0.8, 0.5, 0.0]])
    return np.concatenate((v, ear)), np.concatenate((f, [[0, 1, len(v)]])), len(v)


def bow_tie(n=3):
    """Two flat discs (grid(n)) that share one corner vertex, which so has four border edges.  Returns (v, f, the shared vertex)."""
    v, f = R.grid(n)
    v2 = v + (n - 1.0)
    v2[:, 2] = 0.0
    shared = n * n - 1
    f2 = f + n * n - 1                                                          # the second disc's vertex 0 is the first's last
    return np.concatenate((v, v2[1:])), np.concatenate((f, f2)), shared


# ---- the coned complex and the link condition -------------------------------------------------------------------------------------------
def vertex_classes(V, edges, count):
    """interior / border / locked, from edge_count over a vertex's incident edges."""
    ones, bad = np.zeros(V, dtype=np.int64), np.zeros(V, dtype=bool)
    for side in (0, 1):
        np.add.at(ones, edges[:, side], count == 1)
        bad[edges[(count != 1) & (count != 2), side]] = True
    cls = np.full(V, INTERIOR)
    cls[ones == 2] = BORDER
    cls[bad | ((ones != 0) & (ones != 2))] = LOCKED
    return cls


def coned_complex(V, faces, he2e, count):
    """The faces of the surface closed by a cone: the real ones, then (q, p, W) with W = V for every half-edge p -> q of count 1."""
    a, b = faces.reshape(-1), faces[:, [1, 2, 0]].reshape(-1)
    border = count[he2e] == 1
    cone = np.stack((b[border], a[border], np.full(int(border.sum()), V)), 1)
    return np.concatenate((faces.astype(np.int64), cone.astype(np.int64)))


class Links:
    """Per vertex of a complex: its faces, its neighbours and the edges of its link."""

    def __init__(self, n, faces):
        self.faces = [[] for _ in range(n)]
        self.nbr = [set() for _ in range(n)]
        self.link = [set() for _ in range(n)]
        for i, (a, b, c) in enumerate(faces.tolist()):
            for x, y, z in ((a, b, c), (b, c, a), (c, a, b)):
                self.faces[x].append(i)
                self.nbr[x].update((y, z))
                self.link[x].add((min(y, z), max(y, z)))


def link_condition(V, faces, edges, he2e, count, subset=None):
    """(ok (E,) bool, apexes (E, 2) int64 with -1 for the imaginary one): the closed link condition on the coned complex."""
    E = edges.shape[0]
    cls = vertex_classes(V, edges, count)
    if subset is not None:                      # only the faces that the subset's edges, their neighbours and their apexes see
        near = np.isin(faces, edges[subset]).any(1)
        near = np.isin(faces, faces[near]).any(1)
        faces, he2e = faces[near], he2e.reshape(-1, 3)[near].reshape(-1)
    coned = coned_complex(V, faces, he2e, count)
    K, real = Links(V + 1, coned), Links(V, faces.astype(np.int64))
    ok, apexes = np.zeros(E, dtype=bool), np.full((E, 2), -1, dtype=np.int64)
    coned = [tuple(face) for face in coned.tolist()]
    for e in (range(E) if subset is None else subset):
        u, v = int(edges[e, 0]), int(edges[e, 1])
        if not u < v or count[e] not in (1, 2) or cls[u] == LOCKED or cls[v] == LOCKED:
            continue
        both = [i for i in K.faces[u] if v in coned[i]]
        opposite = [int(x) for i in both for x in coned[i] if x != u and x != v]
        # (a) the link of the edge is two distinct vertices, and the links of u and v share those vertices and nothing else
        if len(both) != 2 or len(opposite) != 2 or opposite[0] == opposite[1] or (K.nbr[u] & K.nbr[v]) != set(opposite):
            continue
        # (b) ... and no edge (the link of the edge holds none)
        if K.link[u] & K.link[v]:
            continue
        apex = [x for x in opposite if x != V]
        # today's stricter form of (b) for two real apexes: no other face of u OR v holds both
        if len(apex) == 2 and ((min(apex), max(apex)) in real.link[u] or (min(apex), max(apex)) in real.link[v]):
            continue
        # (c) the coned valence of every real apex; a locked apex counts its real faces only
        if any((len(real.faces[a]) if cls[a] == LOCKED else len(K.faces[a])) <= 3 for a in apex):
            continue
        # (d) ... and so does the merged vertex, which loses the edge's two faces from either star
        if len(K.faces[u]) + len(K.faces[v]) - 4 <= 3:
            continue
        ok[e] = True
        apexes[e, :len(apex)] = apex
    return ok, apexes


# ---- the header's arithmetic ------------------------------------------------------------------------------------------------------------
def ref_border_quadrics(pos, faces, offsets, corners, he2e, count, border_weight=1.0):
    V, F = pos.shape[0], faces.shape[0]
    p0, p1, p2 = pos[faces[:, 0]], pos[faces[:, 1]], pos[faces[:, 2]]
    c = R.cross(p1 - p0, p2 - p0)
    length = np.sqrt(R.dot(c, c))
    good = length > ZERO
    with np.errstate(invalid="ignore", divide="ignore"):
        n = c / length[:, None]
        d = -R.dot(n, p0)
        w = length / 2.0
        p = np.concatenate((n, d[:, None]), 1)
        qf = np.stack([(w * p[:, a]) * p[:, b] for a in range(4) for b in range(a, 4)], 1)
        # one plane per half-edge 3 f + k, from faces[f][k] to faces[f][(k + 1) % 3]
        a_, b_ = pos[faces.reshape(-1)], pos[faces[:, [1, 2, 0]].reshape(-1)]
        nh = np.repeat(n, 3, 0)
        edge = b_ - a_
        m = R.cross(edge, nh)
        ml = np.sqrt(R.dot(m, m))
        m = m / ml[:, None]
        dh = -R.dot(m, a_)
        wh = np.float64(border_weight) * R.dot(edge, edge)
        ph = np.concatenate((m, dh[:, None]), 1)
        qh = np.stack([(wh * ph[:, a]) * ph[:, b] for a in range(4) for b in range(a, 4)], 1)
    qf = np.where(good[:, None], qf, 0.0)
    qh = np.where((np.repeat(good, 3) & (count[he2e] == 1) & (ml > ZERO))[:, None], qh, 0.0)
    o = offsets.astype(np.int64)
    valence = np.diff(o)
    Q = np.zeros((V, 10))
    for j in range(int(valence.max())):
        vs = np.nonzero(valence > j)[0]
        cn = corners[o[vs] + j].astype(np.int64)
        f, k = cn // 3, cn % 3
        Q[vs] = Q[vs] + qf[f]
        Q[vs] = Q[vs] + qh[cn]                                                 # the corner's outgoing half-edge
        Q[vs] = Q[vs] + qh[3 * f + (k + 2) % 3]                                # its incoming half-edge
    return Q


def ref_border_edges(pos, Q, faces, offsets, corners, edges, he2e, count, subset=None):
    V, E = pos.shape[0], edges.shape[0]
    cand, cost, key = np.zeros((E, 3)), np.zeros(E), np.full(E, NO_KEY, dtype=np.int64)
    passed, apexes = link_condition(V, faces, edges, he2e, count, subset)
    idx = np.nonzero(passed)[0]
    if idx.size == 0:
        return cand, cost, key
    ui, vi = edges[idx, 0].astype(np.int64), edges[idx, 1].astype(np.int64)
    a0, a1 = apexes[idx, 0], apexes[idx, 1]
    # position and cost: am_decimate_edges' expressions
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
        solved = (np.abs(det) > COND * ((tr * tr) * tr)) & (R.dot(off, off) <= REACH * R.dot(edge, edge))
        cy = R.quadric_cost(q, y)
    cu, cv, cm = R.quadric_cost(q, pu), R.quadric_cost(q, pv), R.quadric_cost(q, mid)
    x, cx = pu.copy(), cu.copy()
    better = cv < cx
    x[better], cx[better] = pv[better], cv[better]
    better = cm < cx
    x[better], cx[better] = mid[better], cm[better]
    x[solved], cx[solved] = y[solved], cy[solved]
    cx = np.where(cx > 0.0, cx, 0.0)
    cand[idx], cost[idx] = x, cx
    # no flip over every face of u without v and of v without u
    good = np.ones(idx.size, dtype=bool)
    for s_, o_ in ((ui, vi), (vi, ui)):
        rep, _, fc, k, w1, w2 = R._expand(offsets, corners, faces, s_)
        other = ~((w1 == o_[rep]) | (w2 == o_[rep]))
        p = pos[faces[fc]]
        c0 = R.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        p[np.arange(rep.shape[0]), k] = x[rep]
        c1 = R.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        fine = R.dot(c0, c1) > (FLIP * np.sqrt(R.dot(c0, c0))) * np.sqrt(R.dot(c1, c1))
        good &= np.bincount(rep, weights=other & ~fine, minlength=idx.size) == 0
    bits = cx.astype(np.float32).view(np.uint32).astype(np.uint64)
    k64 = ((bits << np.uint64(32)) | R.mix32(idx)).astype(np.int64)
    key[idx[good]] = k64[good]
    return cand, cost, key


def validate_border(V, faces, offsets, corners, he2e, count, edges=None):
    """R.validate's bits plus what the border kernels add: a half-edge entry outside the edge list, a count below 1 and - with the
    edge list, as am_decimate_border_edges sees it - a count that the faces contradict."""
    bits = R.validate(V, faces, offsets, corners, edges, he2e if edges is not None else None)
    E = count.shape[0]
    if ((he2e < 0) | (he2e >= E)).any() or (count < 1).any():
        bits |= BAD_EDGE
    elif edges is not None and not bits and (np.bincount(he2e, minlength=E) != count).any():
        bits |= BAD_EDGE
    return bits


class NumpyBorderBackend(R.NumpyBackend):
    """R.NumpyBackend with the two border kernels restated."""

    def border_quadrics(self, positions, faces, topology, half_edge_to_edge, edge_count, border_weight=1.0, flag=None):
        V = positions.shape[0]
        f, o, c, h, n = faces.numpy(), topology.offsets.numpy(), topology.corners.numpy(), half_edge_to_edge.numpy(), edge_count.numpy()
        if self._flag(flag, validate_border(V, f, o, c, h, n), V):
            return torch.zeros((V, 10), dtype=torch.float64)
        return torch.from_numpy(ref_border_quadrics(positions.numpy(), f, o, c, h, n, border_weight))

    def border_edges(self, positions, quadrics, faces, topology, edges, half_edge_to_edge, edge_count, flag=None):
        V, E = positions.shape[0], edges.shape[0]
        f, o, c, h, n = faces.numpy(), topology.offsets.numpy(), topology.corners.numpy(), half_edge_to_edge.numpy(), edge_count.numpy()
        if self._flag(flag, validate_border(V, f, o, c, h, n, edges.numpy()), V):
            return torch.zeros((E, 3), dtype=torch.float64), torch.zeros(E, dtype=torch.float64), torch.full((E,), int(NO_KEY))
        return tuple(torch.from_numpy(t) for t in ref_border_edges(positions.numpy(), quadrics.numpy(), f, o, c, edges.numpy(), h, n))


# ---- invariants -------------------------------------------------------------------------------------------------------------------------
def border_loops(f):
    """The border loops as lists of vertices, following the border half-edges (those whose reverse is no half-edge)."""
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    have = set(zip(a.tolist(), b.tolist()))
    nxt = {}
    for p, q in have:
        if (q, p) not in have:
            assert p not in nxt, "two border half-edges leave one vertex"
            nxt[p] = q
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, p = [], start
        while p not in seen:
            seen.add(p)
            loop.append(p)
            p = nxt[p]
        assert p == start, "a border path does not close"
        loops.append(loop)
    return loops


def components(f):
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in f.tolist():
        parent[find(a)] = find(b)
        parent[find(b)] = find(c)
    return len({find(x) for x in list(parent)})


def check_open_manifold(v, f, chi, loops, n_components=1):
    """Every edge in one or two faces and every directed edge once, no repeated index, no duplicate or degenerate face, every vertex
    used, the Euler characteristic, the number of border loops (each of three edges or more) and of connected components."""
    assert np.isin(R.edge_use(f)[1], (1, 2)).all()
    directed = np.stack((f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)), 1)
    assert np.unique(directed, axis=0).shape[0] == directed.shape[0]
    assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 2] != f[:, 0]).all()
    assert np.unique(np.sort(f, 1), axis=0).shape[0] == f.shape[0]
    assert (R.face_areas(v, f) > 0).all()
    assert np.array_equal(np.unique(f), np.arange(v.shape[0]))
    assert R.euler(v.shape[0], f) == chi
    found = border_loops(f)
    assert len(found) == loops and all(len(loop) >= 3 for loop in found)
    assert components(f) == n_components


def border_curve_distance(v0, f0, v1, f1, per_edge=8):
    """The symmetric mean distance between the border polylines: points sampled evenly on every border edge of one mesh, each to the
    nearest point of the other's border segments."""
    def segments(v, f):
        return [(v[p], v[q]) for loop in border_loops(f) for p, q in zip(loop, loop[1:] + loop[:1])]

    def samples(segs):
        t = (np.arange(per_edge) + 0.5) / per_edge
        return np.concatenate([p[None] + (q - p)[None] * t[:, None] for p, q in segs])

    def to_segments(points, segs):
        p = np.stack([s[0] for s in segs])
        d = np.stack([s[1] for s in segs]) - p
        rel = points[:, None, :] - p[None]
        t = np.clip((rel * d[None]).sum(-1) / (d * d).sum(-1)[None], 0.0, 1.0)
        return np.sqrt(((rel - t[..., None] * d[None]) ** 2).sum(-1)).min(1)

    s0, s1 = segments(v0, f0), segments(v1, f1)
    return 0.5 * (to_segments(samples(s0), s1).mean() + to_segments(samples(s1), s0).mean())


# ---- the sequential yardstick -----------------------------------------------------------------------------------------------------------
def greedy_border_decimate(v, f, target_faces, border_weight=1.0):
    """R.greedy_decimate with the border rules: one collapse at a time, the cheapest edge whose stored cost is still its cost, with
    the quadrics, the topology, the placement and the no-flip test of ref_border_quadrics / ref_border_edges."""
    V = v.shape[0]
    pos, faces = v.astype(np.float64).copy(), f.astype(np.int32).copy()

    def tables():
        return R.np_topology(faces, V) + R.np_edges(faces, V)

    t = tables()
    Q = ref_border_quadrics(pos, faces, t[0], t[1], t[3], t[4], border_weight)
    heap = []

    def push(t, subset):
        _, cost, key = ref_border_edges(pos, Q, faces, *t, subset=subset)
        for e in np.nonzero(key != NO_KEY)[0]:
            heapq.heappush(heap, (float(cost[e]), int(t[2][e, 0]), int(t[2][e, 1])))

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
        cand, cost, key = ref_border_edges(pos, Q, faces, *t, subset=np.array([e]))
        if key[e] == NO_KEY:
            continue
        if float(cost[e]) != c0:
            heapq.heappush(heap, (float(cost[e]), a, b))
            continue
        dead = R.ref_apply(pos, Q, faces, t[0], t[1], t[2], cand, np.array([e]), np.arange(V))
        faces = faces[dead == 0]
        reseeded = False
        t = tables()
        push(t, np.nonzero((t[2][:, 0] == a) | (t[2][:, 1] == a))[0])
    return _compact(pos, faces)
