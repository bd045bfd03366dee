"""The yardstick of tests/test_dualcubes_*.py: the dual-marching-cubes contract of include/actionmesh_amd.h (am_dmc_cells,
am_dmc_classify, am_dmc_vertices, am_dmc_triangles) restated in numpy, vectorised over the grid - plus the mesh checks that
tests/_isosurface_ref.py lacks (every vertex's link is one cycle; the number of flipped faces).  The fields and the other topology
helpers are that module's.

The tables are DERIVED here, at import, from the header's geometric rule (segments on the six faces, cycles of segments, the flipped
face); the kernels carry theirs as constants, so a typing error in either shows up in the bit-for-bit comparison.  numpy rounds every
product and every sum on its own (one ufunc call each, no fma), which is the header's arithmetic."""
import numpy as np
import torch

from _isosurface_ref import POPCOUNT, _states

# the twelve cell edges: corner pairs (a, b), a < b, that differ in one bit, in ascending (a, b)
EDGES = [(a, b) for a in range(8) for b in range(a + 1, 8) if bin(a ^ b).count("1") == 1]
EDGE_ID = {e: n for n, e in enumerate(EDGES)}
AXIS_BIT = (4, 2, 1)                                               # the corner-code bit of axis i, j, k


def _face_cycle(axis, side):
    """The four corners of face 2 axis + side in cyclic order."""
    u, v = AXIS_BIT[(axis + 1) % 3], AXIS_BIT[(axis + 2) % 3]
    return [side * AXIS_BIT[axis] + d for d in (0, u, u + v, v)]


FACE_CYCLES = [_face_cycle(axis, side) for axis in range(3) for side in range(2)]


def _patches(cfg, flip_mask=0):
    """(patch of every edge or 255, number of patches, 6-bit mask of ambiguous faces, 6-bit mask of double faces) of one
    configuration, the faces of `flip_mask` cutting off their outside corners."""
    inside = [cfg >> m & 1 for m in range(8)]
    crossing = [inside[a] != inside[b] for a, b in EDGES]
    joined = {e: [] for e in range(12) if crossing[e]}
    two_segments = {}
    for f, cyc in enumerate(FACE_CYCLES):
        fe = [EDGE_ID[tuple(sorted((cyc[n], cyc[(n + 1) % 4])))] for n in range(4)]         # edge n joins corners n and n + 1
        cr = [e for e in fe if crossing[e]]
        assert len(cr) in (0, 2, 4)
        if len(cr) == 2:
            segments = [tuple(cr)]
        elif len(cr) == 4:
            cut_off = 0 if flip_mask >> f & 1 else 1                                       # inside corners by default
            segments = [(fe[n - 1], fe[n]) for n in range(4) if inside[cyc[n]] == cut_off]  # the two face edges at corner n
            assert len(segments) == 2
            two_segments[f] = segments
        else:
            segments = []
        for a, b in segments:
            joined[a].append(b)
            joined[b].append(a)
    patch = [255] * 12
    count = 0
    for e in range(12):                                            # ascending: patches are numbered by their smallest edge
        if not crossing[e] or patch[e] != 255:
            continue
        stack = [e]
        while stack:
            x = stack.pop()
            if patch[x] == 255:
                patch[x] = count
                stack.extend(joined[x])
        count += 1
    assert all(len(v) == 2 for v in joined.values())               # every crossing edge lies on two faces: cycles
    ambiguous = sum(1 << f for f in two_segments)
    double = sum(1 << f for f, s in two_segments.items() if patch[s[0][0]] == patch[s[1][0]])
    return patch, count, ambiguous, double


def _derive_tables():
    """PATCH (2, 256, 12): the patch of every edge (255: it does not cross) by the default rule and with the double face flipped
    (the default row again where there is none); NPATCH (2, 256); AMBIGUOUS, DOUBLE (256,): 6-bit face masks, face 2 axis + side."""
    patch, npatch = np.full((2, 256, 12), 255, dtype=np.uint8), np.zeros((2, 256), dtype=np.int64)
    ambiguous, double = np.zeros(256, dtype=np.uint8), np.zeros(256, dtype=np.uint8)
    for cfg in range(256):
        patch[0, cfg], npatch[0, cfg], ambiguous[cfg], double[cfg] = _patches(cfg)
        patch[1, cfg], npatch[1, cfg] = _patches(cfg, int(double[cfg]))[:2]
    return patch, npatch, ambiguous, double


PATCH, NPATCH, AMBIGUOUS, DOUBLE = _derive_tables()


def _steps(shape):
    X, Y, Z = shape
    return np.array([((m >> 2 & 1) * Y + (m >> 1 & 1)) * Z + (m & 1) for m in range(8)], dtype=np.int64)


def ref_cells(values, level=0.0, inside_above=True):
    """(config, double), both (X, Y, Z) uint8, at the point of the cell's 000 corner: the inside mask of an ACTIVE cell (0 anywhere
    else) and the mask of its double faces."""
    X, Y, Z = values.shape
    finite, inside = _states(values, level, inside_above)
    all_finite = np.ones((X - 1, Y - 1, Z - 1), dtype=bool)
    cfg = np.zeros((X - 1, Y - 1, Z - 1), dtype=np.int64)
    for m in range(8):
        di, dj, dk = m >> 2 & 1, m >> 1 & 1, m & 1
        all_finite &= finite[di:X - 1 + di, dj:Y - 1 + dj, dk:Z - 1 + dk]
        cfg |= inside[di:X - 1 + di, dj:Y - 1 + dj, dk:Z - 1 + dk].astype(np.int64) << m
    cfg[~all_finite | (cfg == 255)] = 0
    config = np.zeros(values.shape, dtype=np.uint8)
    config[:-1, :-1, :-1] = cfg
    return config, DOUBLE[config]


def ref_classify(config, double):
    """(code int16, count uint8, edge_mask uint8), all (X, Y, Z): config + 256 when the cell's double face is flipped; its number
    of patches; bit `axis` for the edge from p along `axis` that emits a quad."""
    shape = config.shape
    flip = np.zeros(shape, dtype=bool)
    for axis in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3              # the cell and its neighbour on the high side of `axis`
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        both = ((double[lo] >> (2 * axis + 1) & 1) & (double[hi] >> (2 * axis) & 1)).astype(bool)
        flip[lo] |= both
        flip[hi] |= both
    code = config.astype(np.int16) | (flip.astype(np.int16) << 8)
    count = NPATCH[flip.astype(np.int64), config].astype(np.uint8)
    active = config != 0
    mask = np.zeros(shape, dtype=np.uint8)
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        around = active.copy()                                     # all four cells around the edge exist and are ACTIVE
        for du, dv in ((1, 0), (1, 1), (0, 1)):
            shifted = np.zeros(shape, dtype=bool)
            src, dst = [slice(None)] * 3, [slice(None)] * 3
            if du:
                src[u], dst[u] = slice(0, -1), slice(1, None)
            if dv:
                src[v], dst[v] = slice(0, -1), slice(1, None)
            shifted[tuple(dst)] = active[tuple(src)]
            around &= shifted
        crosses = (config & 1) != (config >> AXIS_BIT[axis] & 1)             # corner 000 against the corner along the axis
        mask |= (around & crosses).astype(np.uint8) << axis
    return code, count, mask


def offsets_of(count, edge_mask):
    """The caller's plumbing: (vertex_offset, tri_offset) int64 (X, Y, Z) and the two totals."""
    cnt = count.reshape(-1).astype(np.int64)
    tri = 2 * POPCOUNT[edge_mask.reshape(-1)]
    return (np.cumsum(cnt) - cnt).reshape(count.shape), (np.cumsum(tri) - tri).reshape(count.shape), int(cnt.sum()), int(tri.sum())


def ref_vertices(values, code, vertex_offset, n_vertices, origin, spacing, level=0.0):
    """(n_vertices, 3) fp32: the dual vertex of patch q of cell p at vertex_offset[p] + q."""
    shape = values.shape
    flat_code = code.reshape(-1).astype(np.int64)
    cells = np.nonzero(flat_code)[0]
    cfg, flip = flat_code[cells] & 255, flat_code[cells] >> 8
    patch = PATCH[flip, cfg]                                                               # (N, 12)
    idx0 = np.stack(np.unravel_index(cells, shape), axis=1)
    v = values.astype(np.float64).reshape(-1)
    step = _steps(shape)
    org, sp = np.asarray(origin, dtype=np.float64), np.asarray(spacing, dtype=np.float64)
    total = np.zeros((4, cells.shape[0], 3), dtype=np.float64)
    number = np.zeros((4, cells.shape[0]), dtype=np.int64)
    with np.errstate(all="ignore"):
        for e, (a, b) in enumerate(EDGES):                                                 # ascending edge id
            va, vb = v[cells + step[a]], v[cells + step[b]]
            t = (level - va) / (vb - va)
            pa = org + (idx0 + np.array([a >> 2 & 1, a >> 1 & 1, a & 1])).astype(np.float64) * sp
            pb = org + (idx0 + np.array([b >> 2 & 1, b >> 1 & 1, b & 1])).astype(np.float64) * sp
            x = pa + t[:, None] * (pb - pa)
            for q in range(4):
                sel = patch[:, e] == q
                total[q] = np.where(sel[:, None], total[q] + x, total[q])
                number[q] += sel
    out = np.zeros((n_vertices, 3), dtype=np.float32)
    base = vertex_offset.reshape(-1)[cells]
    for q in range(4):
        sel = number[q] > 0
        out[base[sel] + q] = (total[q][sel] / number[q][sel, None].astype(np.float64)).astype(np.float32)
    return out


def ref_triangles(code, edge_mask, vertex_offset, tri_offset, vertices, n_vertices, n_triangles):
    """(n_triangles, 3) int32: two per emitting edge, ordered by 3 p + axis."""
    shape = code.shape
    flat_code, flat_mask = code.reshape(-1).astype(np.int64), edge_mask.reshape(-1)
    flat_voff, flat_toff = vertex_offset.reshape(-1), tri_offset.reshape(-1)
    step = (shape[1] * shape[2], shape[2], 1)
    pos = vertices.astype(np.float64)
    out = np.zeros((n_triangles, 3), dtype=np.int32)
    for axis in range(3):
        p = np.nonzero(flat_mask >> axis & 1)[0]
        u, v = (axis + 1) % 3, (axis + 2) % 3
        quad = []
        for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):                                    # around the edge
            cell = p - du * step[u] - dv * step[v]
            a = du * AXIS_BIT[u] + dv * AXIS_BIT[v]                                        # the corner of that cell at p
            c = flat_code[cell]
            patch = PATCH[c >> 8, c & 255][:, EDGE_ID[(a, a + AXIS_BIT[axis])]]
            assert (patch != 255).all()
            quad.append(flat_voff[cell] + patch)
        q = np.stack(quad, axis=1)
        lower_inside = (flat_code[p] & 1) != 0
        q[~lower_inside] = q[~lower_inside][:, [0, 3, 2, 1]]                               # the normal: from the inside to the outside
        d02, d13 = pos[q[:, 0]] - pos[q[:, 2]], pos[q[:, 1]] - pos[q[:, 3]]
        l02 = (d02[:, 0] * d02[:, 0] + d02[:, 1] * d02[:, 1]) + d02[:, 2] * d02[:, 2]
        l13 = (d13[:, 0] * d13[:, 0] + d13[:, 1] * d13[:, 1]) + d13[:, 2] * d13[:, 2]
        second = l13 < l02                                                                 # a tie goes to first - third
        row = flat_toff[p] + 2 * POPCOUNT[flat_mask[p] & ((1 << axis) - 1)]
        out[row] = np.where(second[:, None], q[:, [0, 1, 3]], q[:, [0, 1, 2]])
        out[row + 1] = np.where(second[:, None], q[:, [1, 2, 3]], q[:, [0, 2, 3]])
    return out


def ref_tables(values, level=0.0, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), inside_above=True):
    """Every intermediate result of the extraction, by name."""
    s = {}
    s["config"], s["double"] = ref_cells(values, level, inside_above)
    s["code"], s["count"], s["emask"] = ref_classify(s["config"], s["double"])
    s["voff"], s["toff"], s["V"], s["F"] = offsets_of(s["count"], s["emask"])
    if s["V"] and s["F"]:
        s["vertices"] = ref_vertices(values, s["code"], s["voff"], s["V"], origin, spacing, level)
        s["faces"] = ref_triangles(s["code"], s["emask"], s["voff"], s["toff"], s["vertices"], s["V"], s["F"])
    return s


def ref_extract(values, level=0.0, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), inside_above=True, compact=True):
    """The whole extraction: (vertices (V, 3) fp32, faces (F, 3) int64), unused vertices dropped when `compact`."""
    s = ref_tables(values, level, origin, spacing, inside_above)
    if s["V"] == 0 or s["F"] == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)
    vertices, faces = s["vertices"], s["faces"].astype(np.int64)
    if compact:
        used = np.zeros(s["V"], dtype=bool)
        used[faces.reshape(-1)] = True
        vertices, faces = vertices[used], (np.cumsum(used) - 1)[faces]
    return vertices, faces


def flipped_faces(values, level=0.0, inside_above=True):
    """The number of flipped faces: every one is flipped in the two cells that share it."""
    code = ref_classify(*ref_cells(values, level, inside_above))[0]
    flipped = int((code >> 8).sum())
    assert flipped % 2 == 0
    return flipped // 2


def ref_extract_without_flips(values, level=0.0):
    """What the default rule alone gives (index frame, not compacted): the mesh the flip is there to repair."""
    s = {}
    s["config"], s["double"] = ref_cells(values, level)
    s["code"], s["count"], s["emask"] = ref_classify(s["config"], np.zeros_like(s["double"]))
    voff, toff, V, F = offsets_of(s["count"], s["emask"])
    vertices = ref_vertices(values, s["code"], voff, V, (0.0,) * 3, (1.0,) * 3, level)
    return vertices, ref_triangles(s["code"], s["emask"], voff, toff, vertices, V, F).astype(np.int64)


class NumpyBackend:
    """The restatement behind the interface of `actionmesh_amd.isosurface.HipDualBackend`, on CPU tensors."""

    @staticmethod
    def cells(values, level=0.0, inside_above=True):
        return tuple(torch.from_numpy(a) for a in ref_cells(values.numpy(), level, inside_above))

    @staticmethod
    def classify(config, double):
        return tuple(torch.from_numpy(a) for a in ref_classify(config.numpy(), double.numpy()))

    @staticmethod
    def vertices(values, code, vertex_offset, n_vertices, origin, spacing, level=0.0, inside_above=True, flag=None):
        return torch.from_numpy(ref_vertices(values.numpy(), code.numpy(), vertex_offset.numpy(), n_vertices, origin, spacing, level))

    @staticmethod
    def triangles(code, edge_mask, vertex_offset, tri_offset, vertices, n_vertices, n_triangles, flag=None):
        return torch.from_numpy(ref_triangles(code.numpy(), edge_mask.numpy(), vertex_offset.numpy(), tri_offset.numpy(),
                                              vertices.numpy(), n_vertices, n_triangles))


# ---- mesh checks ---------------------------------------------------------------------------------------------------------------------
def vertices_whose_link_is_not_one_cycle(n_vertices, faces):
    """The vertices whose link - the edges opposite to them in their faces - is anything but one closed cycle."""
    nxt = [dict() for _ in range(n_vertices)]
    bad = set()
    for a, b, c in faces.tolist():
        for v, s, t in ((a, b, c), (b, c, a), (c, a, b)):
            if s in nxt[v]:
                bad.add(v)
            nxt[v][s] = t
    for v, link in enumerate(nxt):
        if v in bad or not link:
            bad.add(v)
            continue
        start = at = next(iter(link))
        for steps in range(1, len(link) + 1):
            at = link.get(at)
            if at is None or at == start:
                break
        if at != start or steps != len(link):
            bad.add(v)
    return sorted(bad)


def edges_in_more_than_two_faces(faces):
    from _isosurface_ref import edge_use_counts
    return int((edge_use_counts(faces) > 2).sum())


def check_manifold(vertices, faces, chi=None):
    """Closed, oriented, every vertex used and its link one cycle; the Euler characteristic when given."""
    from _isosurface_ref import all_vertices_used, directed_edges_unique, edge_use_counts, euler
    uses = edge_use_counts(faces)
    assert (uses == 2).all(), f"{(uses != 2).sum()} edges are not in exactly two faces"
    assert directed_edges_unique(faces) and all_vertices_used(vertices.shape[0], faces)
    assert vertices_whose_link_is_not_one_cycle(vertices.shape[0], faces) == []
    if chi is not None:
        assert euler(vertices.shape[0], faces) == chi
