"""The yardstick of tests/test_isosurface_*.py: the iso-surface contract of include/actionmesh_amd.h (am_iso_classify, am_iso_vertices,
am_iso_triangles) restated in numpy, vectorised over the grid - plus the analytic fields and the topology helpers of those tests.

The case table is DERIVED here, at import, from the header's geometric rule (polygon by corner order, reversed when its normal on the
unit tetrahedron points from the outside corners to the inside ones); the kernel carries its table as constants, so a typing error in
either shows up in the bit-for-bit comparison.  numpy rounds every product and every sum on its own (one ufunc call each, no fma),
which is the header's arithmetic."""
import itertools

import numpy as np
import torch

PERMS = list(itertools.permutations(range(3)))                     # lexicographic: tetrahedron 0 .. 5
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def _tet_corners(perm):
    corners = [np.zeros(3, dtype=np.int64)]
    for axis in perm:
        nxt = corners[-1].copy()
        nxt[axis] = 1
        corners.append(nxt)
    return corners                                                 # c0 = 000, c1 = c0 + e_pi0, c2 = c1 + e_pi1, c3 = 111


def _code(offset):
    return int(offset[0]) * 4 + int(offset[1]) * 2 + int(offset[2])     # (di, dj, dk), dk lowest


def _derive_table():
    """CORNER (6, 4): the offset codes of every tetrahedron's corners.  TRI_COUNT (6, 16) and TRI_EDGE (6, 16, 2, 3, 2): for the
    inside mask of (c0 .. c3), the triangles as (corner a, corner b) pairs with a < b."""
    corner = np.array([[_code(c) for c in _tet_corners(p)] for p in PERMS], dtype=np.int64)
    count, edge = np.zeros((6, 16), dtype=np.int64), np.zeros((6, 16, 2, 3, 2), dtype=np.int64)
    for t, perm in enumerate(PERMS):
        pos = [c.astype(np.float64) for c in _tet_corners(perm)]
        for case in range(1, 15):
            ins = [q for q in range(4) if case >> q & 1]
            out = [q for q in range(4) if not case >> q & 1]
            if len(ins) == 1:
                poly = [(ins[0], o) for o in out]
            elif len(ins) == 3:
                poly = [(i, out[0]) for i in ins]
            else:
                poly = [(ins[0], out[0]), (ins[0], out[1]), (ins[1], out[1]), (ins[1], out[0])]
            mid = [0.5 * (pos[a] + pos[b]) for a, b in poly]
            towards_outside = sum(pos[o] for o in out) / len(out) - sum(pos[i] for i in ins) / len(ins)
            if np.cross(mid[1] - mid[0], mid[2] - mid[0]) @ towards_outside < 0:
                poly = [poly[0]] + poly[:0:-1]
            tris = [poly] if len(poly) == 3 else [[poly[0], poly[1], poly[2]], [poly[0], poly[2], poly[3]]]
            count[t, case] = len(tris)
            for n, tri in enumerate(tris):
                edge[t, case, n] = [sorted(e) for e in tri]
    return corner, count, edge


CORNER, TRI_COUNT, TRI_EDGE = _derive_table()


def _states(values, level, inside_above):
    v = values.astype(np.float64)
    finite = np.isfinite(v)
    with np.errstate(invalid="ignore"):
        inside = finite & ((v > level) if inside_above else (v < level))
    return finite, inside


def _shifted(a, m, fill):
    """a[i + di, j + dj, k + dk] at every point, `fill` where that leaves the grid."""
    di, dj, dk = m >> 2 & 1, m >> 1 & 1, m & 1
    out = np.full(a.shape, fill, dtype=a.dtype)
    X, Y, Z = a.shape
    out[:X - di, :Y - dj, :Z - dk] = a[di:, dj:, dk:]
    return out


def ref_classify(values, level=0.0, inside_above=True):
    """(mask, count), both (X, Y, Z) uint8."""
    finite, inside = _states(values, level, inside_above)
    fin = [_shifted(finite, m, False) for m in range(8)]
    ins = [_shifted(inside, m, False) for m in range(8)]
    mask = np.zeros(values.shape, dtype=np.uint8)
    for m in range(1, 8):
        mask |= (fin[0] & fin[m] & (ins[0] != ins[m])).astype(np.uint8) << (m - 1)
    count = np.zeros(values.shape, dtype=np.int64)
    for t in range(6):
        c = CORNER[t]
        all_finite = fin[c[0]] & fin[c[1]] & fin[c[2]] & fin[c[3]]
        case = sum(ins[c[q]].astype(np.int64) << q for q in range(4))
        count += np.where(all_finite, TRI_COUNT[t][case], 0)
    return mask, count.astype(np.uint8)


def offsets_of(mask, count):
    """The caller's plumbing: (vertex_offset, tri_offset) int64 (X, Y, Z) and the two totals."""
    pop = POPCOUNT[mask.reshape(-1)]
    cnt = count.reshape(-1).astype(np.int64)
    return ((np.cumsum(pop) - pop).reshape(mask.shape), (np.cumsum(cnt) - cnt).reshape(mask.shape), int(pop.sum()), int(cnt.sum()))


def ref_vertices(values, mask, vertex_offset, n_vertices, origin, spacing, level=0.0):
    """(n_vertices, 3) fp32: one vertex per crossing edge, in ascending edge id 7 p + (m - 1)."""
    X, Y, Z = values.shape
    flat_mask = mask.reshape(-1)
    points = np.nonzero(flat_mask)[0]
    bits = (flat_mask[points, None] >> np.arange(7)) & 1
    row, col = np.nonzero(bits)                                    # row-major: ascending p, then ascending m
    p, m = points[row], col + 1
    rank = POPCOUNT[flat_mask[p] & ((1 << (m - 1)) - 1)]
    dest = vertex_offset.reshape(-1)[p] + rank
    idx_a = np.stack(np.unravel_index(p, (X, Y, Z)), axis=1)
    idx_b = idx_a + np.stack((m >> 2 & 1, m >> 1 & 1, m & 1), axis=1)
    v = values.astype(np.float64)
    va, vb = v[tuple(idx_a.T)], v[tuple(idx_b.T)]
    t = (level - va) / (vb - va)
    org, sp = np.asarray(origin, dtype=np.float64), np.asarray(spacing, dtype=np.float64)
    pa = org + idx_a.astype(np.float64) * sp
    pb = org + idx_b.astype(np.float64) * sp
    out = np.zeros((n_vertices, 3), dtype=np.float32)
    out[dest] = (pa + t[:, None] * (pb - pa)).astype(np.float32)
    return out


def ref_triangles(values, mask, count, vertex_offset, tri_offset, n_vertices, n_triangles, level=0.0, inside_above=True):
    """(n_triangles, 3) int32: ordered by cell, tetrahedron, triangle."""
    X, Y, Z = values.shape
    finite, inside = _states(values, level, inside_above)
    cells = np.nonzero(count.reshape(-1))[0]
    ci, cj, ck = np.unravel_index(cells, (X, Y, Z))
    step = np.array([((m >> 2 & 1) * Y + (m >> 1 & 1)) * Z + (m & 1) for m in range(8)], dtype=np.int64)
    corner_p = cells[:, None] + step[None, :]                                            # (N, 8) linear indices
    fin, ins = finite.reshape(-1)[corner_p], inside.reshape(-1)[corner_p]
    flat_mask, flat_off = mask.reshape(-1), vertex_offset.reshape(-1)
    faces = np.zeros((cells.shape[0], 6, 2, 3), dtype=np.int64)
    valid = np.zeros((cells.shape[0], 6, 2), dtype=bool)
    for t in range(6):
        c = CORNER[t]
        all_finite = fin[:, c].all(axis=1)
        case = sum(ins[:, c[q]].astype(np.int64) << q for q in range(4))
        n = np.where(all_finite, TRI_COUNT[t][case], 0)
        for tri in range(2):
            valid[:, t, tri] = n > tri
            for corner in range(3):
                a, b = TRI_EDGE[t, case, tri, corner, 0], TRI_EDGE[t, case, tri, corner, 1]
                code_a, code_b = c[a], c[b]
                m = np.maximum(code_b - code_a, 1)                                      # 1 where the slot is unused
                pa = corner_p[np.arange(cells.shape[0]), code_a]
                faces[:, t, tri, corner] = flat_off[pa] + POPCOUNT[flat_mask[pa] & ((1 << (m - 1)) - 1)]
    out = faces[valid]
    assert out.shape[0] == n_triangles and np.array_equal(valid.sum(axis=(1, 2)), count.reshape(-1)[cells])
    assert (np.cumsum(valid.sum(axis=(1, 2))) - valid.sum(axis=(1, 2)) == tri_offset.reshape(-1)[cells]).all()
    return out.astype(np.int32)


def ref_extract(values, level=0.0, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), inside_above=True, compact=True):
    """The whole extraction: (vertices (V, 3) fp32, faces (F, 3) int64), unused vertices dropped when `compact`."""
    mask, count = ref_classify(values, level, inside_above)
    voff, toff, V, F = offsets_of(mask, count)
    if V == 0 or F == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)
    vertices = ref_vertices(values, mask, voff, V, origin, spacing, level)
    faces = ref_triangles(values, mask, count, voff, toff, V, F, level, inside_above).astype(np.int64)
    if compact:
        used = np.zeros(V, dtype=bool)
        used[faces.reshape(-1)] = True
        vertices, faces = vertices[used], (np.cumsum(used) - 1)[faces]
    return vertices, faces


class NumpyBackend:
    """The restatement behind the interface of `actionmesh_amd.isosurface.HipBackend`, on CPU tensors."""

    @staticmethod
    def classify(values, level=0.0, inside_above=True):
        mask, count = ref_classify(values.numpy(), level, inside_above)
        return torch.from_numpy(mask), torch.from_numpy(count)

    @staticmethod
    def vertices(values, mask, vertex_offset, n_vertices, origin, spacing, level=0.0, flag=None):
        return torch.from_numpy(ref_vertices(values.numpy(), mask.numpy(), vertex_offset.numpy(), n_vertices, origin, spacing, level))

    @staticmethod
    def triangles(values, mask, count, vertex_offset, tri_offset, n_vertices, n_triangles, level=0.0, inside_above=True, flag=None):
        return torch.from_numpy(ref_triangles(values.numpy(), mask.numpy(), count.numpy(), vertex_offset.numpy(), tri_offset.numpy(),
                                              n_vertices, n_triangles, level, inside_above))


# ---- fields: float64 on np.linspace(-1, 1, n), indexing "ij", cast to float32 -------------------------------------------------------
SPHERE_CENTRE, SPHERE_RADIUS = (0.03, -0.02, 0.01), 0.8
TORUS_MAJOR, TORUS_MINOR = 0.6, 0.25


def axes(n, lo=-1.0, hi=1.0):
    x = np.linspace(lo, hi, n)
    return np.meshgrid(x, x, x, indexing="ij")


def frame(n, lo=-1.0, hi=1.0):
    """(origin, spacing) of the n^3 grid between lo and hi."""
    return (lo,) * 3, ((hi - lo) / (n - 1),) * 3


def sphere_of(x, y, z, radius=SPHERE_RADIUS, centre=SPHERE_CENTRE):
    return radius - np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)


def torus_of(x, y, z):
    return TORUS_MINOR - np.sqrt((np.sqrt(x ** 2 + y ** 2) - TORUS_MAJOR) ** 2 + z ** 2)


def sphere(n):
    return sphere_of(*axes(n)).astype(np.float32)


def torus(n):
    return torus_of(*axes(n)).astype(np.float32)


def two_spheres(n):
    x, y, z = axes(n)
    return np.maximum(sphere_of(x, y, z, 0.3, (0.5, 0.0, 0.0)), sphere_of(x, y, z, 0.3, (-0.5, 0.0, 0.0))).astype(np.float32)


def octahedron():
    i, j, k = np.meshgrid(*(np.arange(9),) * 3, indexing="ij")
    return (3 - (abs(i - 4) + abs(j - 4) + abs(k - 4))).astype(np.float32)


def noncubic_with_nans():
    """5 x 9 x 17, an off-centre ellipsoid, three samples not evaluated; with its anisotropic frame."""
    i, j, k = np.meshgrid(np.arange(5), np.arange(9), np.arange(17), indexing="ij")
    v = (1.0 - np.sqrt(((i - 2.1) / 1.7) ** 2 + ((j - 3.9) / 3.2) ** 2 + ((k - 8.3) / 6.4) ** 2)).astype(np.float32)
    v[2, 4, 2], v[1, 1, 8], v[3, 7, 11] = np.nan, np.inf, -np.inf
    return v, (-0.3, 0.1, 2.0), (0.37, 0.11, 0.052)


SPHERE_VOLUME = 4.0 / 3.0 * np.pi * SPHERE_RADIUS ** 3
TORUS_VOLUME = 2.0 * np.pi ** 2 * TORUS_MAJOR * TORUS_MINOR ** 2


# ---- topology ----------------------------------------------------------------------------------------------------------------------
def edge_use_counts(faces):
    """The number of faces on every undirected edge."""
    e = np.sort(np.stack((faces, faces[:, [1, 2, 0]]), axis=-1).reshape(-1, 2), axis=1)
    return np.unique(e, axis=0, return_counts=True)[1]


def euler(n_vertices, faces):
    return n_vertices - edge_use_counts(faces).shape[0] + faces.shape[0]


def directed_edges_unique(faces):
    d = np.stack((faces, faces[:, [1, 2, 0]]), axis=-1).reshape(-1, 2)
    return np.unique(d, axis=0).shape[0] == d.shape[0]


def all_vertices_used(n_vertices, faces):
    return np.unique(faces).shape[0] == n_vertices


def signed_volume(vertices, faces):
    v = vertices.astype(np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def face_normals_and_areas(vertices, faces):
    v = vertices.astype(np.float64)
    n = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    return n, 0.5 * np.linalg.norm(n, axis=1)


def check_closed_oriented(vertices, faces, chi):
    uses = edge_use_counts(faces)
    assert (uses == 2).all(), f"{(uses != 2).sum()} edges are not in exactly two faces"
    assert directed_edges_unique(faces) and all_vertices_used(vertices.shape[0], faces)
    assert euler(vertices.shape[0], faces) == chi
