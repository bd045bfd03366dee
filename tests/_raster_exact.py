"""Scenes on which am_render_normals (csrc/am_raster.hip) has ONE correct answer at every sub-pixel, the integer reference that
states it, and the comparison the GPU test and the CPU test share.  Nothing of the kernel's arithmetic is here: coverage, depth
order and vertex normals are decided by Python / NumPy integers.

The lattice.  W = 2S sub-pixels a side, S a power of two.  A sub-pixel centre is 1 - (2i + 1) / W = (W - 1 - 2i) / W: an odd integer
over W.  Every vertex is placed so that it projects to an integer over W as well ("lattice units" below): cameras have a signed
permutation R that keeps the z axis (any other one puts the planes below edge-on to the camera), T = (0, 0, 2), an integer focal length and a principal point of integers over W; a vertex of
the plane at view depth z in {1, 2, 4} has view x, y = k z / W.  World coordinates are integers over W (`verts`), so that the
projection k f + m is exact in fp32 and here.  Every difference and product inside the edge function is then an integer number of
1 / W^2 below 2^24: exact in fp32.  The sign or zero of every unclipped barycentric is the sign or zero of an integer, and

    covered       all three edge integers strictly on the area's side,
    not covered   any edge integer 0 (a centre on an edge or on a vertex), or a zero area,
    the box       implied: a centre strictly inside a triangle in front of the camera is inside its closed box.

A rasterised face lies in one plane parallel to the image (but for the scene "straddle": see _straddler), so its interpolated depth is within a few ulp of z and the planes 1, 2, 4
order with certainty.  Two faces of one plane may cover a common centre only when their three projected vertices are the same rows
in the same order: their z-buffer keys then have the same depth bits and the lower index wins.

Normals.  The vertex normal of a planar patch parallel to the image is (0, 0, +-1) in view space, and soft_normal_shading maps the
view normal n to n + (0, 0, 1): a patch whose normal points away from the camera (+z) shows exactly (0.5, 0.5, 1), the normal 0 of
an uncovered sub-pixel does too, and a patch that looks straight at the camera (-z) gives (0, 0, 1 - sigma) with sigma the fp32 sum
of the barycentrics - zero up to rounding, a direction no reference can state.  `tilt()` therefore gives such a patch auxiliary
faces (P + d, P, lambda P): they lie in a plane through the camera's centre, project to a segment (two of the three projections are
bit-identical, so the area is exactly 0 and the raster skips them), and their un-normalised normal cancels the patch's z at the
vertex P and leaves an exact multiple of +-x or +-y.  The tilted patch shows (1 +- 1/sqrt 2) / 2 in that channel: a third and fourth
colour, so a normal read from the wrong sub-pixel shows.  `conditions()` asserts that every output pixel of every scene is of one of
the stated kinds.  A patch that looks away and the n = 0 of an uncovered sub-pixel cannot differ in colour: both are +z after the
shading.

The closed box of the header cannot be told from an open one by any face in front of the camera (a centre strictly inside a
triangle is strictly inside its box), so the scene "straddle" has faces with vertices at depth -1 and +1 - still on the lattice,
still decided by integers (_straddler) - whose cone of positive barycentrics reaches centres on the box's edges."""
import itertools
from fractions import Fraction

import numpy as np

U = 2.0 ** -24                       # unit roundoff of fp32
BARY_C = 7                           # roundings between the exact E_i / A and a written barycentric: see compare()
NORMAL_C = 6.5                       # |normal - fp64| <= NORMAL_C * U on a tilted patch: see compare()
PLANES = (1, 2, 4)
IDENTITY = ((1, 0, 0), (0, 1, 0), (0, 0, 1))
ROT90 = ((0, 1, 0), (-1, 0, 0), (0, 0, 1))       # view = X @ R: world x -> view y, world y -> view -x
ROT180 = ((-1, 0, 0), (0, -1, 0), (0, 0, 1))


def camera(R=IDENTITY, f=1, p=(0, 0)):
    """R: signed permutation that keeps z; f: integer focal length; p: principal point in lattice units (integers over W)."""
    return {"R": tuple(tuple(int(x) for x in r) for r in R), "f": int(f), "p": (int(p[0]), int(p[1]))}


def torch_camera(cam, W):
    import torch
    return {"R": torch.tensor(cam["R"], dtype=torch.float32), "T": torch.tensor([0.0, 0.0, 2.0]),
            "focal_length": torch.tensor([float(cam["f"])] * 2), "principal_point": torch.tensor([cam["p"][0] / W, cam["p"][1] / W])}


def float_verts(scene):
    """(T, V, 3) fp32: integers over W, exact."""
    v = scene["verts"].astype(np.float64) / (2 * scene["S"])
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    return v.astype(np.float32)


# ---- building -------------------------------------------------------------------------------------------------------------
class Builder:
    """Vertices are given in the lattice units of the identity camera with f = 1, p = 0 (view space: x, y = k z / W at depth z) and
    kept as world integers over W (world = view - T).  `away=True` orders a face so that its view normal is +z (it looks away from
    the camera), False so that it looks at it; `away=None` keeps the order given."""

    def __init__(self, name, S):
        self.name, self.S, self.W = name, S, 2 * S
        self.v, self.f = [], []

    def vert(self, kx, ky, z):
        self.v.append((kx * z, ky * z, (z - 2) * self.W))
        return len(self.v) - 1

    def _normal_z(self, i0, i1, i2):
        a, b = np.subtract(self.v[i2], self.v[i1]), np.subtract(self.v[i0], self.v[i1])
        return int(a[0] * b[1] - a[1] * b[0])

    def face(self, i0, i1, i2, away=True):
        if away is not None and self._normal_z(i0, i1, i2) != 0 and (self._normal_z(i0, i1, i2) > 0) != away:
            i1, i2 = i2, i1
        self.f.append((i0, i1, i2))
        return len(self.f) - 1

    def tri(self, k0, k1, k2, z, away=True):
        """A triangle on three vertices of its own."""
        return self.face(*(self.vert(k[0], k[1], z) for k in (k0, k1, k2)), away=away)

    def grid(self, xs, ys, z, away=True):
        """A lattice patch on shared vertices: nodes xs x ys, every cell split along alternating diagonals."""
        ids = [[self.vert(x, y, z) for x in xs] for y in ys]
        out = []
        for j, i in itertools.product(range(len(ys) - 1), range(len(xs) - 1)):
            a, b, c, d = ids[j][i], ids[j][i + 1], ids[j + 1][i + 1], ids[j + 1][i]
            out += [self.face(a, b, c, away), self.face(a, c, d, away)] if (i + j) % 2 == 0 else \
                   [self.face(a, b, d, away), self.face(b, c, d, away)]
        return out, [i for row in ids for i in row]

    def tilt(self, vertex_ids, axis=0):
        """See the module docstring.  For the vertex P with patch normal (0, 0, a): the face (P + d, P, lambda P), d along the other
        image axis than `axis`, lambda = 2 (1/2 in the farthest plane), has the normal (lambda - 1) P x d; d is chosen so that its z
        is -a, which leaves a P_z / P_axis along `axis`.  Everything is an integer over W or the builder refuses."""
        W = self.W
        for i in vertex_ids:
            P = self.v[i]
            a = sum(self._normal_z(*f) for f in self.f for k in f if k == i)
            z = P[2] // W + 2
            lam = Fraction(2) if z <= 2 else Fraction(1, 2)
            assert a != 0 and P[axis] != 0, (i, a, P)
            # axis 0: d = (0, dy, 0), (P x d).z = P_x dy;  axis 1: d = (dx, 0, 0), (P x d).z = -P_y dx
            step = Fraction(-a if axis == 0 else a) / ((lam - 1) * P[axis])
            assert step.denominator == 1 and int(step) % z == 0, ("tilt leaves the lattice", i, step, z)
            q = list(P)
            q[1 - axis] += int(step)
            view = (P[0], P[1], z * W)
            L = tuple(Fraction(x) * lam for x in view)
            assert all(x.denominator == 1 for x in L)
            iq = len(self.v)
            self.v += [tuple(q), (int(L[0]), int(L[1]), int(L[2]) - 2 * W)]
            self.f.append((iq, i, iq + 1))

    def scene(self, cams=None, shifts=((0, 0),)):
        """`shifts`: one lattice translation per frame, in units of 4 / W of world x, y (4, 2 and 1 lattice units in the planes 1, 2, 4)."""
        v = np.array(self.v, dtype=np.int64)
        verts = np.stack([v + np.array([4 * sx, 4 * sy, 0]) for sx, sy in shifts])
        return {"name": self.name, "S": self.S, "verts": verts, "faces": np.array(self.f, dtype=np.int64),
                "cams": list(cams) if cams else [camera()]}


# ---- the scenes ------------------------------------------------------------------------------------------------------------
def scene_tiling():
    """S = 16.  A 5 x 5-node patch with nodes three lattice units apart (odd and even alternate, so edges, diagonals and vertices pass
    through centres) looking away; the same patch looking at the camera, tilted; single faces of both orientations that share an
    edge through centres on vertices of their own; zero-area lattice triangles (three collinear vertices, a repeated vertex) and
    slivers between two neighbouring columns / rows of centres."""
    b = Builder("tiling", 16)
    b.grid((3, 6, 9, 12, 15), (2, 5, 8, 11, 14), 1)
    # the facing patch: columns 4, 8, 16 and rows 8 apart keep every tilt on the lattice; its 8 x 8 cells' diagonals pass centres
    _, ids = b.grid((-16, -8, -4), (-24, -16, -8), 2, away=False)
    b.tilt(ids, axis=0)
    # two facing triangles on their own vertices sharing the edge (-3, 5) - (-9, 11) (centres (-5, 7), (-7, 9) lie on it; vertices
    # on centres), tilted along x;  cross = 36 = 2 * 18, a multiple of 3 and 9
    n0 = len(b.v)
    b.tri((-3, 5), (-9, 5), (-9, 11), 1, away=False)
    b.tri((-3, 5), (-9, 11), (-3, 11), 1, away=False)
    b.tilt(range(n0, n0 + 6), axis=0)
    # the same pair looking away, sharing an edge whose end points are centres
    b.tri((5, -5), (11, -5), (11, -11), 1)
    b.tri((5, -5), (11, -11), (5, -11), 1)
    # a facing pair below the axis, tilted along y (cross = 64, rows -8 and -16)
    n0 = len(b.v)
    b.tri((17, -8), (25, -8), (25, -16), 1, away=False)
    b.tri((17, -8), (25, -16), (17, -16), 1, away=False)
    b.tilt(range(n0, n0 + 6), axis=1)
    # a facing pair right of the axis (+x is the left of the image), where the tilt lands on -x (cross = 32, columns 4 and 8)
    n0 = len(b.v)
    b.tri((4, -30), (8, -30), (8, -22), 1, away=False)
    b.tri((4, -30), (8, -22), (4, -22), 1, away=False)
    b.tilt(range(n0, n0 + 6), axis=0)
    # zero areas: collinear lattice points through centres, and a repeated position
    b.tri((-29, 21), (-25, 25), (-21, 29), 1, away=None)
    b.tri((15, 21), (15, 21), (21, 27), 1, away=None)
    # slivers: between the centre columns 21 and 23 / the rows 21 and 23, and a slanted one that passes between centres
    b.tri((22, 15), (22, 29), (22 + 1, 15), 2, away=None)        # x in [22, 23): touches column 23 only on its vertex
    b.tri((-15, 22), (-1, 22), (-15, 22 + 1), 2, away=None)
    b.tri((-30, -30), (-18, -30), (-30, -29), 4)
    return b.scene()


def scene_border():
    """S = 16: boxes whose edges are centres; faces over the sub-pixel rows and columns 0 and W - 1; faces partly and wholly outside
    on each side; corners; one face behind the camera that would otherwise fill the frame."""
    b = Builder("border", 16)
    b.tri((5, 5), (11, 5), (5, 11), 1)                         # box edges and vertices on centres
    b.tri((-4, -5), (-8, -5), (-4, -13), 2, away=False)        # looking at the camera (tilted): box rows on centres
    b.tilt(range(3, 6), axis=0)
    for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):        # corners: the extreme centre (+-31, +-31) strictly inside / on the edge
        b.tri((sx * 33, sy * 33), (sx * 25, sy * 33), (sx * 33, sy * 25), 1)
    b.tri((31, 17), (31, 23), (25, 17), 1)                     # box edge on column 0's centres: an edge through them covers none
    b.tri((-31, -17), (-31, -23), (-25, -17), 1)
    b.tri((13, 31), (19, 31), (13, 25), 2)
    b.tri((-13, -31), (-19, -31), (-13, -25), 2)
    for k, (ax, s) in enumerate(((0, 1), (0, -1), (1, 1), (1, -1))):       # the four sides: partly and wholly outside
        def at(u, w):
            return (s * u, w) if ax == 0 else (w, s * u)
        o = -9 + 6 * k if ax == 0 else 1 + 4 * k
        b.tri(at(28, o), at(40, o), at(28, o + 5), 1)
        b.tri(at(36, o), at(48, o), at(36, o + 5), 2)
        b.tri(at(32, o - 8), at(44, o - 8), at(32, o - 4), 4)              # its edge ON the image border, between no centres
    b.tri((-40, -40), (40, -40), (0, 40), -1)                              # behind the camera
    return b.scene()


def scene_depth():
    """S = 16: three overlapping triangles in the planes 1, 2, 4 in each of the six index orders; identical duplicates at a low and
    a high index (the same vertex rows, and a copy on vertices of its own at the same positions); a big-path face with a nearer and
    a farther small-path face inside it."""
    b = Builder("depth", 16)
    dup_first = b.tri((-29, 13), (-15, 13), (-29, 27), 1)
    spots = [(-27, -27), (-5, -27), (15, -27), (-27, -5), (-5, -5), (15, -5)]
    for (x, y), order in zip(spots, itertools.permutations(PLANES)):
        for z in order:
            o = {1: 0, 2: 3, 4: 6}[z]
            b.tri((x + o, y + o), (x + o + 12, y + o), (x + o, y + o + 12), z)
    big = b.tri((-7, 11), (15, 11), (-7, 31), 2)               # 11 x 10 centres: queued
    b.tri((-3, 15), (3, 15), (-3, 21), 1)                      # nearer and small
    b.tri((1, 13), (9, 13), (1, 19), 4)                        # farther and small: hidden where the big face covers
    b.tri((17, 13), (29, 13), (17, 25), 4)
    b.face(*b.f[-1], away=None)                                # a tie in the farthest plane, the duplicate at the higher index
    v = [b.vert(*k, 1) for k in ((-29, 13), (-15, 13), (-29, 27))]
    b.face(*v, away=True)                                      # positions of face 0 on rows of their own
    b.face(*b.f[dup_first], away=None)                         # face 0 again at the highest index
    assert big > 0
    return b.scene()


def scene_paths():
    """S = 32.  A right triangle with legs of 2k lattice units has k + 1 centres a side when its corner is a centre and k when it is
    not; pix_range adds one sub-pixel on either side of an odd bound and one and two of an even one, so the loop box is (k + 3)^2 in
    both cases: k = 2 .. 8 gives 5 x 5 .. 11 x 11.  8 x 8 = 64 = SMALL_BOX is the last the raster thread tests itself, 9 x 9 = 81 the
    first that is queued.  The thin ones: 2k x 4 lattice units, loop boxes (k + 3) x 5 = 65 / 80 / 100 for k = 10, 13, 17 (queued)
    and 60 for k = 9 (not queued), each wide, tall, and wide with the corner between centres."""
    b = Builder("paths", 32)
    x = -59
    for n, k in enumerate(range(2, 9)):
        for odd in (1, 0):
            cx, cy = x - (1 - odd), 43 - 21 * (1 - odd)                  # corner (odd, 43) on a centre, (even, 22) between centres
            b.tri((cx, cy), (cx + 2 * k, cy), (cx, cy + 2 * k), PLANES[n % 3])
        x += 2 * k + 4
    for n, k in enumerate((9, 10, 13, 17)):
        y = 5 - 8 * n
        b.tri((-61, y), (-61 + 2 * k, y), (-61, y + 4), PLANES[n % 3])                      # wide
        b.tri((-15 + 8 * n, -61), (-15 + 8 * n + 4, -61), (-15 + 8 * n, -61 + 2 * k), 1)     # tall
        b.tri((60 - 2 * k, y), (60, y), (60, y + 4), 2)                                     # wide, corner between centres
    return b.scene()


QUEUE_CAMS = (camera(), camera(ROT90), camera(ROT180, f=2, p=(6, -10)))


def scene_queue():
    """S = 32, T = 2 frames (the second moved by (8, -4) / W in world x, y) x C = 3 cameras (rotations about the axis by 0, 90 and
    180 degrees, the last with focal 2 and the principal point (6, -10) / W), F = 1101.  25 spots x 3 planes of right triangles with
    18-unit legs (12 x 12 loop boxes: queued), each plane's triangle moved by (2, 2) against the nearer one, every triangle stacked
    14 or 15 times on the same vertex rows, the index order of the planes changing from spot to spot: 6606 queue entries."""
    b = Builder("queue", 32)
    base = []
    for j, i in itertools.product(range(5), range(5)):
        x, y = -61 + 25 * i, -61 + 25 * j
        base.append([(b.vert(x + o, y + o, z), b.vert(x + o + 18, y + o, z), b.vert(x + o, y + o + 18, z))
                     for z, o in zip(PLANES, (0, 2, 4))])
    orders = list(itertools.permutations(range(3)))
    n = 0
    while len(b.f) < 1101:
        for s, tris in enumerate(base):
            if len(b.f) < 1101:
                b.face(*tris[orders[(s + n // 3) % 6][n % 3]])
        n += 1
    return b.scene(QUEUE_CAMS, shifts=((0, 0), (2, -1)))


def scene_straddle():
    """S = 16, fragments only (no normal is stated: these faces are not parallel to the image).  Faces with two vertices behind the
    camera (depth -1) and one in front, whose front vertex projects extreme on neither axis: the cone beyond it in which all three
    barycentrics are positive runs through the box of the projected vertices to its edges, which lie on centres - covered under the
    closed box of include/actionmesh_amd.h, not under an open one - and on outside it, where nothing is covered.  The same with
    one vertex behind: the interpolated depth is negative in the whole cone and nothing is covered."""
    b = Builder("straddle", 16)
    for (ox, oy), zs in (((-10, -10), (-1, -1, 1)), ((12, 8), (-1, -1, 1)), ((-12, 12), (1, 1, -1))):
        pts = ((ox - 15, oy - 9), (ox + 9, oy + 15), (ox + 1, oy + 3))
        if ox > 0:
            pts = tuple((ox - (y - oy), oy + (x - ox)) for x, y in pts)             # a quarter turn: the cone opens upwards
        b.face(*(b.vert(x, y, z) for (x, y), z in zip(pts, zs)), away=None)
    s = b.scene()
    s["fragments_only"] = True
    return s


SCENES = {"straddle": scene_straddle, "tiling": scene_tiling, "border": scene_border, "depth": scene_depth, "paths": scene_paths, "queue": scene_queue}


# ---- the integer reference -------------------------------------------------------------------------------------------------
def _edge(px, py, a, b):
    return (px - a[0]) * (b[1] - a[1]) - (py - a[1]) * (b[0] - a[0])


def _straddler(E, A, zf, X, Y, lo, hi, facts):
    """Coverage of a face with depths +-1 on both sides of the camera plane, E and A already signed so that A > 0.  The header's
    t_i = w_i z_j z_k is T_i / A' with the integers T_i = E_i z_j z_k (A' the area with its 1e-8); their sum is D / A'.  A sum that is
    not positive is replaced by 1e-8 and leaves some p_i <= 0, so: covered when D > 0, every T_i > 0, the centre is inside the CLOSED
    box and the interpolated depth sum(T_i z_i) / D = A z_0 z_1 z_2 / D is not negative - never, then, with one vertex behind the
    camera.  fp32 decides the same: every t_i carries one rounding of a magnitude below 2^13 / A against |D| / A >= 1 / A, and the
    depth is at least A / |D| > 2^-16 from zero (asserted)."""
    T = E * np.array([zf[1] * zf[2], zf[0] * zf[2], zf[0] * zf[1]])
    D = T.sum(-1)
    assert np.abs(T).max() < 2 ** 13 and A * 2 ** 16 > np.abs(D).max()
    cone = (D > 0) & (T > 0).all(-1) & (zf[0] * zf[1] * zf[2] > 0)
    inbox = (X >= lo[0]) & (X <= hi[0]) & (Y >= lo[1]) & (Y <= hi[1])
    on_box = inbox & ((X == lo[0]) | (X == hi[0]) | (Y == lo[1]) | (Y == hi[1]))
    facts["cone_on_box_edge"] = facts.get("cone_on_box_edge", 0) + int((cone & on_box).sum())
    facts["cone_outside_box"] = facts.get("cone_outside_box", 0) + int((cone & ~inbox).sum())
    facts["depth_rejected"] = facts.get("depth_rejected", 0) + int(((D > 0) & (T > 0).all(-1) & inbox & ~cone).sum())
    return cone & inbox


def project(scene, t, c):
    """Lattice coordinates K (V, 2) and depth z (V,) of frame t under camera c: integers, or an AssertionError."""
    W, cam = 2 * scene["S"], scene["cams"][c]
    R = np.array(cam["R"], dtype=np.int64)
    assert sorted(np.abs(R).sum(0).tolist()) == [1, 1, 1] and sorted(np.abs(R).sum(1).tolist()) == [1, 1, 1] and R[2, 2] == 1
    view = scene["verts"][t] @ R + np.array([0, 0, 2 * W])
    assert (view[:, 2] % W == 0).all(), "a vertex between the planes"
    z = view[:, 2] // W
    assert np.isin(z, (-1,) + PLANES).all(), "view depth outside {-1, 1, 2, 4}"
    num = cam["f"] * view[:, :2]
    assert (num % z[:, None] == 0).all(), "a vertex off the lattice"
    K = num // z[:, None] + np.array(cam["p"])
    assert np.abs(K).max() < 2 ** 12 and np.abs(view).max() < 2 ** 20
    return K, z


def vertex_normals(scene, t):
    """The un-normalised vertex normals of frame t (world space) in units of 1 / W^2: sums of cross(v2 - v1, v0 - v1), integers.  Every
    product and partial sum is asserted below 2^24, so the kernel's fp32 sums are these integers and sqrt(n . n) of an axis-aligned
    one is its magnitude exactly."""
    V, F = scene["verts"][t], scene["faces"]
    a, b = V[F[:, 2]] - V[F[:, 1]], V[F[:, 0]] - V[F[:, 1]]
    assert max(np.abs(a).max(), np.abs(b).max()) ** 2 < 2 ** 23
    fn = np.cross(a, b)
    n = np.zeros_like(V)
    mag = np.zeros(len(V), dtype=np.int64)
    for k in range(3):
        np.add.at(n, F[:, k], fn)
        np.add.at(mag, F[:, k], np.abs(fn).max(1))
    assert mag.max() < 2 ** 24
    return n


def image(scene, t, c):
    """The reference of image (t, c).  Raises where a premise of the module docstring fails."""
    S = scene["S"]
    W = 2 * S
    F = scene["faces"]
    K, z = project(scene, t, c)
    xs = W - 1 - 2 * np.arange(W)                                   # lattice coordinate of column / row i
    X, Y = np.meshgrid(xs, xs)                                      # [row, col]
    face = np.full((W, W), -1, dtype=np.int64)
    depth = np.full((W, W), 99, dtype=np.int64)
    num = np.zeros((W, W, 3), dtype=np.int64)
    den = np.zeros((W, W), dtype=np.int64)
    rows_of = {}
    owner = {p: np.full((W, W), -1, dtype=np.int64) for p in PLANES}
    hits = np.zeros((W, W), dtype=np.int64)
    straddled = np.zeros((W, W), dtype=bool)                        # won by a face with vertices on both sides of the camera plane
    strict = np.zeros(len(F), dtype=np.int64)                       # centres each face strictly covers, whoever wins them
    facts = {"rasterised": 0, "on_edge": 0, "ties": 0, "max_product": 0, "zero_area": 0, "behind": 0}
    for f, (i0, i1, i2) in enumerate(F):
        v0, v1, v2 = K[i0], K[i1], K[i2]
        if max(z[i0], z[i1], z[i2]) < 0:
            facts["behind"] += 1
            continue
        A = int(_edge(v2[0], v2[1], v0, v1))
        if A == 0:
            facts["zero_area"] += 1
            continue
        zf = (int(z[i0]), int(z[i1]), int(z[i2]))
        planar = zf[0] == zf[1] == zf[2] and zf[0] > 0
        assert planar or (scene.get("fragments_only") and set(zf) == {-1, 1}), f"face {f} is rasterised and not parallel to the image"
        lo, hi = np.minimum(np.minimum(v0, v1), v2), np.maximum(np.maximum(v0, v1), v2)
        reach = W - 1 + np.maximum(np.abs(lo), np.abs(hi))
        prod = int(max(reach[0] * (hi[1] - lo[1]), reach[1] * (hi[0] - lo[0])))
        facts["max_product"] = max(facts["max_product"], prod)
        assert 2 * prod < 2 ** 24 and abs(A) < 2 ** 24
        facts["rasterised"] += 1
        E = np.stack([_edge(X, Y, v1, v2), _edge(X, Y, v2, v0), _edge(X, Y, v0, v1)], -1) * (1 if A > 0 else -1)
        if not planar:
            cov = _straddler(E, abs(A), zf, X, Y, lo, hi, facts)
            assert (hits[cov] == 0).all(), f"face {f} straddles the camera plane and overlaps another face"
            hits += cov
            straddled |= cov
            strict[f] = int(cov.sum())
            face[cov], depth[cov] = f, 0
            continue
        assert (E.sum(-1) == abs(A)).all()
        cov = (E > 0).all(-1)
        facts["on_edge"] += int(((E >= 0).all(-1) & ~cov).sum())
        strict[f] = int(cov.sum())
        hits += cov
        if not cov.any():
            continue
        # the box rule is implied
        assert (X[cov] >= lo[0]).all() and (X[cov] <= hi[0]).all() and (Y[cov] >= lo[1]).all() and (Y[cov] <= hi[1]).all()
        key = (tuple(v0), tuple(v1), tuple(v2))
        rid = rows_of.setdefault(key, len(rows_of))
        own = owner[int(z[i0])]
        assert ((own[cov] == -1) | (own[cov] == rid)).all(), f"face {f} overlaps another face of its plane"
        facts["ties"] += int((own[cov] == rid).sum())
        own[cov] = rid
        closer = cov & (z[i0] < depth)                              # strict: a tie stays with the lower index
        face[closer], depth[closer], den[closer] = f, z[i0], abs(A)
        num[closer] = E[closer]
    # ---- resolve
    assert (hits[straddled] == 1).all()
    covered = face >= 0
    mask_q = covered.reshape(S, 2, S, 2).sum((1, 3))
    facts["covered"] = int(covered.sum())
    if scene.get("fragments_only"):
        return {"face": face, "num": num, "den": den, "stated": covered & ~straddled, "mask_q": mask_q, "strict": strict,
                "facts": facts, "alpha": np.floor(mask_q / 4.0 * 255).astype(np.int64)}
    Rm = np.array(scene["cams"][c]["R"], dtype=np.int64)
    vn = vertex_normals(scene, t)
    axis_like = (vn != 0).sum(1) <= 1
    assert (np.abs(vn).max(1)[(vn != 0).any(1)] > 1e-6 * W * W).all()
    unit = np.sign(vn) @ Rm                                         # view space; meaningful where axis_like
    f00 = face[::2, ::2]
    tri = F[np.maximum(f00, 0)]                                     # (S, S, 3)
    shown = f00 >= 0
    assert axis_like[tri[shown]].all(), "a shown vertex normal is not along an axis"
    e = np.where(shown[..., None, None], unit[tri], 0)              # (S, S, 3 corners, 3)
    g_num = (num[::2, ::2][..., None] * e).sum(2)                   # exact n = g_num / den, per pixel
    d00 = np.maximum(den[::2, ::2], 1)
    normal = np.empty((S, S, 3))
    kind = np.zeros((S, S), dtype=np.int64)                         # 0: exactly (0.5, 0.5, 1);  1: a tilted patch
    plus_z = (g_num[..., 0] == 0) & (g_num[..., 1] == 0)
    # m_z = 1 + n_z must be positive beyond any rounding: 2^-10 against the 9 * 2^-24 of the sum of the barycentrics
    assert ((g_num[..., 2] + d00)[plus_z] * 1024 >= d00[plus_z]).all(), "a patch looks straight at the camera untilted"
    normal[plus_z] = (0.5, 0.5, 1.0)
    tilted = ~plus_z
    same = (e == e[..., :1, :]).all((2, 3)) & (g_num[..., 2] == 0) & (np.abs(g_num).sum(-1) == d00)
    assert same[tilted].all(), "a shown face mixes vertex normals"
    kind[tilted] = 1
    m = g_num[tilted] / d00[tilted][:, None] + np.array([0.0, 0.0, 1.0])                 # (+-1, 0, 1) or (0, +-1, 1)
    normal[tilted] = (m / np.sqrt(2.0) + 1) / 2
    exact = np.ones((S, S, 3), dtype=bool)
    exact[tilted] = g_num[tilted] == 0                                                   # the 0.5 of the untouched channel
    exact[tilted, 2] = False
    mk = mask_q / 4.0
    value = (normal * mk[..., None] + (1 - mk[..., None])) * 255                          # exact in fp64 where `exact`
    frac = value - np.floor(value)
    margin = np.minimum(frac, 1 - frac)
    assert (margin[~exact] >= 1e-3).all(), "a tilted pixel within 1e-3 of a byte boundary"
    rgba = np.concatenate([np.floor(value), np.floor(mk * 255)[..., None]], -1).astype(np.int64)
    facts.update(covered=int(covered.sum()), tilted=int(tilted.sum()), partial=int(((mask_q > 0) & (mask_q < 4)).sum()),
                 uncovered_shown=int(((mask_q > 0) & ~shown).sum()), colours=len({tuple(x) for x in rgba[mask_q == 4].tolist()}))
    return {"face": face, "num": num, "den": den, "mask_q": mask_q, "normal": normal, "exact": exact, "kind": kind, "rgba": rgba,
            "stated": covered, "strict": strict, "facts": facts}


_cache = {}


def reference(name):
    """scene, {(t, c): image reference}: computed once and shared; callers do not write into it."""
    if name not in _cache:
        scene = SCENES[name]()
        _cache[name] = (scene, {(t, c): image(scene, t, c) for t in range(len(scene["verts"])) for c in range(len(scene["cams"]))})
    return _cache[name]


def conditions(scene):
    """The premises, asserted on the operands alone (image() raises where one fails); returns the facts it counted."""
    S = scene["S"]
    assert S in (16, 32, 64) and scene["verts"].dtype == np.int64 and scene["verts"].ndim == 3
    assert scene["faces"].min() >= 0 and scene["faces"].max() < scene["verts"].shape[1]
    float_verts(scene)
    total = {}
    for t in range(len(scene["verts"])):
        for c in range(len(scene["cams"])):
            for k, v in image(scene, t, c)["facts"].items():
                total[k] = max(total.get(k, 0), v) if k in ("max_product", "colours") else total.get(k, 0) + v
    assert total["max_product"] * 2 < 2 ** 24
    return total


# ---- the comparison --------------------------------------------------------------------------------------------------------
def compare(got, ref, label=""):
    """Every sub-pixel and every pixel of one image (`got`: pix_to_face (W, W), bary (W, W, 3), mask, normal (S, S[, 3]), rgba
    (S, S, 4)) against its reference.  Returns (largest barycentric err / bound, largest tilted-normal err / bound).

    The barycentric bound.  E_i and the area A are exact; cover() then rounds: area + 1e-8 (the same for the three, it cancels in
    p = t / den), w_i = E_i / area (1), t_i = w_i z z (exact: z is a power of two), den = t_0 + t_1 + t_2 (2, the same for the three:
    it cancels in b = c / s), p_i = t_i / den (1), s = p_0 + p_1 + p_2 (2; the maxima against 1e-8, 0 and 1e-5 change nothing: den is
    z^2 >= 1, p > 0, s is 1 up to rounding), b_i = p_i / s (1).  Against s, a weighted mean of the p_j with their 2 roundings each,
    b_i carries 2 + 2 + 2 + 1 = 7 roundings: |b_i - E_i / A| <= gamma_7 E_i / A, gamma_7 = 7u / (1 - 7u), u = 2^-24.

    The tilted normal.  sigma = fl(fl(b_0 + b_1) + b_2) = 1 + theta, |theta| <= 9u (7 of the b, 2 sums); m = (+-sigma, 0, 1) exactly;
    d^2 = fl(fl(sigma^2) + 1): relative (18u + u) / 2 + u = 10.5u against 2; d = sqrt: 5.25u + u; m / d: 9u + 6.25u + u = 16.25u of
    1 / sqrt 2 = 11.5u absolute; + 1 rounds by at most u; halved: 6.25u first order, asserted as 6.5u."""
    W = ref["face"].shape[0]
    face, bary = np.asarray(got["pix_to_face"]).astype(np.int64), np.asarray(got["bary"]).astype(np.float64)
    bad = face != ref["face"]
    assert not bad.any(), f"{label}: pix_to_face differs on {int(bad.sum())} of {W * W} sub-pixels, first at (row, col) " \
                          f"{tuple(np.argwhere(bad)[0])}: got {face[bad][0]}, reference {ref['face'][bad][0]}"
    mask = np.asarray(got["mask"]).astype(np.float64)
    assert np.array_equal(mask * 4, ref["mask_q"]), f"{label}: mask differs"
    assert (bary[ref["face"] < 0] == -1.0).all(), f"{label}: an uncovered sub-pixel's barycentrics are not -1"
    loose = (ref["face"] >= 0) & ~ref["stated"]                     # a straddling face's: positive and summing to 1, no more is stated
    assert (bary[loose] > 0).all() and (np.abs(bary[loose].sum(-1) - 1) <= 4 * U).all()
    cov = ref["stated"]
    n, d = ref["num"][cov].astype(np.float64), ref["den"][cov].astype(np.float64)[:, None]
    gamma = BARY_C * U / (1 - BARY_C * U)
    ratio = np.abs(bary[cov] * d - n) / (gamma * n)                 # |b - E / A| / (gamma E / A): b * A is exact in fp64 (24 + 24 bits)
    worst_b = float(ratio.max()) if ratio.size else 0.0
    assert worst_b <= 1.0, f"{label}: barycentric err / bound {worst_b}"
    rgba = np.asarray(got["rgba"]).astype(np.int64)
    if "normal" not in ref:                                         # a fragments-only scene: the alpha byte alone
        assert np.array_equal(rgba[..., 3], ref["alpha"]), f"{label}: alpha differs"
        return worst_b, 0.0
    normal = np.asarray(got["normal"]).astype(np.float64)
    ex = ref["exact"]
    assert np.array_equal(normal[ex], ref["normal"][ex]), f"{label}: a normal that is exactly 0.5 or 1 differs"
    err = np.abs(normal - ref["normal"])[~ex]
    worst_n = float(err.max() / (NORMAL_C * U)) if err.size else 0.0
    assert worst_n <= 1.0, f"{label}: tilted normal err / bound {worst_n}"
    bad = (rgba != ref["rgba"]).any(-1)
    assert not bad.any(), f"{label}: bytes differ on {int(bad.sum())} pixels, first at {tuple(np.argwhere(bad)[0])}: got " \
                          f"{rgba[bad][0]}, reference {ref['rgba'][bad][0]}"
    return worst_b, worst_n
