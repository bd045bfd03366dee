"""am_render_normals restated op for op in NumPy fp32 from the arithmetic include/actionmesh_amd.h states (and the operation order of
csrc/am_raster.hip, which compiles without contraction): projection, the face rejections, the loop bounds, cover(), the 64-bit
z-buffer key and the resolve.  Only IEEE add, subtract, multiply, divide, min / max and sqrt occur, all correctly rounded in NumPy as
on the device, so pix_to_face, bary and mask are expected bit for bit.  `fault` plants one of the errors the exact scenes exist to
reject (tests/test_raster_exact_cpu.py)."""
import numpy as np

f32 = np.float32
K_EPS = f32(1e-8)
SMALL_BOX = 64
ZB_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
BIG_BLOCKS = 1024
FAULTS = ("ge", "open_box", "tie_high", "transposed_split", "one_stride", "normal_of_last_subpixel")
ONE, HALF, ZERO = f32(1), f32(0.5), f32(0)


def project(X, cam):
    """X (V, 3) fp32 -> (V, 3) {x_ndc, y_ndc, view z}."""
    R, T = np.asarray(cam["R"], dtype=f32).reshape(3, 3), np.asarray(cam["T"], dtype=f32)
    fx, fy = (f32(v) for v in cam["focal_length"])
    px, py = (f32(v) for v in cam["principal_point"])
    q = [X[:, 0] * R[0, j] + X[:, 1] * R[1, j] + X[:, 2] * R[2, j] + T[j] for j in range(3)]
    with np.errstate(all="ignore"):
        return np.stack([fx * q[0] / q[2] + px, fy * q[1] / q[2] + py, q[2]], 1).astype(f32)


def edge_fn(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def cover(v0, v1, v2, px, py, fault=None):
    """v: (..., 3) fp32 broadcastable against px, py.  Returns covered, b (..., 3), z."""
    with np.errstate(all="ignore"):
        x0, x1, x2, y0, y1, y2, z0, z1, z2 = v0[..., 0], v1[..., 0], v2[..., 0], v0[..., 1], v1[..., 1], v2[..., 1], v0[..., 2], \
            v1[..., 2], v2[..., 2]
        lx, hx = np.fmin(np.fmin(x0, x1), x2), np.fmax(np.fmax(x0, x1), x2)
        ly, hy = np.fmin(np.fmin(y0, y1), y2), np.fmax(np.fmax(y0, y1), y2)
        out = (px <= lx) | (px >= hx) | (py <= ly) | (py >= hy) if fault == "open_box" else (px < lx) | (px > hx) | (py < ly) | (py > hy)
        area = edge_fn(x2, y2, x0, y0, x1, y1) + K_EPS
        w0, w1, w2 = edge_fn(px, py, x1, y1, x2, y2) / area, edge_fn(px, py, x2, y2, x0, y0) / area, edge_fn(px, py, x0, y0, x1, y1) / area
        t0, t1, t2 = w0 * z1 * z2, z0 * w1 * z2, z0 * z1 * w2
        den = np.fmax(t0 + t1 + t2, K_EPS)
        p0, p1, p2 = t0 / den, t1 / den, t2 / den
        inside = (p0 >= 0) & (p1 >= 0) & (p2 >= 0) if fault == "ge" else (p0 > 0) & (p1 > 0) & (p2 > 0)
        c0, c1, c2 = np.fmax(p0, ZERO), np.fmax(p1, ZERO), np.fmax(p2, ZERO)
        s = np.fmax(c0 + c1 + c2, f32(1e-5))
        b = np.stack([c0 / s, c1 / s, c2 / s], -1)
        z = b[..., 0] * z0 + b[..., 1] * z1 + b[..., 2] * z2
        return ~out & inside & (z >= 0), b.astype(f32), z.astype(f32)


def ndc_of(i, n):
    return ONE - (2 * i + 1).astype(f32) / f32(n)


def pix_range(a_min, a_max, n):
    with np.errstate(all="ignore"):
        f_lo = ((ONE - a_max) * f32(n) - ONE) * HALF
        f_hi = ((ONE - a_min) * f32(n) - ONE) * HALF
    lo = 0 if not f_lo > 1 else (n if f_lo >= n else int(f_lo) - 1)
    hi = n - 1 if not f_hi < n - 2 else (-1 if f_hi < -1 else int(f_hi) + 1)
    return lo, hi


def face_setup(P, tri, W):
    """None for a rejected face, else (v0, v1, v2, r_lo, r_hi, c_lo, c_hi)."""
    v0, v1, v2 = P[tri[0]], P[tri[1]], P[tri[2]]
    if np.fmax(np.fmax(v0[2], v1[2]), v2[2]) < 0:
        return None
    with np.errstate(all="ignore"):
        a = edge_fn(v0[0], v0[1], v1[0], v1[1], v2[0], v2[1])
    if a <= K_EPS and a >= -K_EPS:
        return None
    c_lo, c_hi = pix_range(np.fmin(np.fmin(v0[0], v1[0]), v2[0]), np.fmax(np.fmax(v0[0], v1[0]), v2[0]), W)
    r_lo, r_hi = pix_range(np.fmin(np.fmin(v0[1], v1[1]), v2[1]), np.fmax(np.fmax(v0[1], v1[1]), v2[1]), W)
    if not (c_lo <= c_hi and r_lo <= r_hi):
        return None
    return v0, v1, v2, r_lo, r_hi, c_lo, c_hi


def queued(P, F, W):
    """The faces raster_small_kernel hands to the queue: loop box above SMALL_BOX sub-pixels."""
    out = []
    for f, tri in enumerate(F):
        s = face_setup(P, tri, W)
        out.append(s is not None and (s[6] - s[5] + 1) * (s[4] - s[3] + 1) > SMALL_BOX)
    return np.array(out)


def vertex_normals(X, F):
    """One vertex at a time in face-index order, as the CSR walk does."""
    n = np.zeros_like(X)
    for i0, i1, i2 in F:
        a, b = X[i2] - X[i1], X[i0] - X[i1]
        fn = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=f32)
        for i in (i0, i1, i2):
            n[i] += fn
    d = np.fmax(np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2]), f32(1e-6))
    return (n / d[:, None]).astype(f32)


def render(X, F, cam, S, fault=None, normals=True, queue_base=0):
    """One image: X (V, 3) fp32, F (F, 3), cam as render.py takes it.  Returns the dict of HipRenderer.render_normals for it.
    `queue_base`: the queue entries of the images before this one, for the fault "one_stride" (raster_big_kernel without its
    `e += gridDim.x`: entries past BIG_BLOCKS are never drawn; the entries are taken in (image, face) order)."""
    assert fault is None or fault in FAULTS
    X = np.ascontiguousarray(X, dtype=f32)
    F = np.asarray(F, dtype=np.int64)
    W = 2 * S
    P = project(X, cam)
    zb = np.full((W, W), ZB_EMPTY, dtype=np.uint64)
    for f, tri in enumerate(F):
        s = face_setup(P, tri, W)
        if s is None:
            continue
        v0, v1, v2, r_lo, r_hi, c_lo, c_hi = s
        bw, bh = c_hi - c_lo + 1, r_hi - r_lo + 1
        if bw * bh > SMALL_BOX:
            queue_base += 1
            if fault == "one_stride" and queue_base > BIG_BLOCKS:
                continue
        r, c = np.meshgrid(np.arange(r_lo, r_hi + 1), np.arange(c_lo, c_hi + 1), indexing="ij")
        if fault == "transposed_split" and bw * bh > SMALL_BOX:
            p = np.arange(bw * bh)
            r, c = r_lo + p % bw, c_lo + p // bw                    # for r_lo + p / bw, c_lo + p % bw
            keep = (r >= 0) & (r < W) & (c >= 0) & (c < W)          # a device would write outside the z-buffer
            r, c = r[keep], c[keep]
        cov, _, z = cover(v0, v1, v2, ndc_of(c, W), ndc_of(r, W), fault)
        bits = np.where(z > 0, z, ZERO).astype(f32).view(np.uint32).astype(np.uint64)
        low = np.uint64(0xFFFFFFFF - f if fault == "tie_high" else f)
        key = (bits << np.uint64(32)) | low
        r, c, key = r[cov], c[cov], key[cov]
        np.minimum.at(zb, (r, c), key)
    face = np.where(zb == ZB_EMPTY, -1, (zb & np.uint64(0xFFFFFFFF)).astype(np.int64))
    if fault == "tie_high":
        face = np.where(zb == ZB_EMPTY, -1, 0xFFFFFFFF - face)
    covered = face >= 0
    rr, cc = np.meshgrid(np.arange(W), np.arange(W), indexing="ij")
    tri = F[np.maximum(face, 0)]
    _, b, _ = cover(P[tri[..., 0]], P[tri[..., 1]], P[tri[..., 2]], ndc_of(cc, W), ndc_of(rr, W), fault)
    bary = np.where(covered[..., None], b, f32(-1)).astype(f32)
    mask = (covered.reshape(S, 2, S, 2).sum((1, 3)).astype(f32) * f32(0.25)).astype(f32)
    out = {"pix_to_face": face.astype(np.int32), "bary": bary, "mask": mask}
    if not normals:
        return out
    vn = vertex_normals(X, F)
    k = 1 if fault == "normal_of_last_subpixel" else 0
    f00, b00, t00 = covered[k::2, k::2], bary[k::2, k::2], tri[k::2, k::2]
    n = [np.where(f00, b00[..., 0] * vn[t00[..., 0], a] + b00[..., 1] * vn[t00[..., 1], a] + b00[..., 2] * vn[t00[..., 2], a], ZERO)
         for a in range(3)]
    R, T = np.asarray(cam["R"], dtype=f32).reshape(3, 3), np.asarray(cam["T"], dtype=f32)
    m = [n[0] * R[0, a] + n[1] * R[1, a] + n[2] * R[2, a] + T[a] * HALF for a in range(3)]
    d = np.fmax(np.sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]), f32(1e-12))
    u = np.stack([np.fmin(np.fmax((m[a] / d + ONE) * HALF, ZERO), ONE) for a in range(3)], -1).astype(f32)
    rgb = ((u * mask[..., None] + (ONE - mask[..., None])) * f32(255)).astype(np.uint8)
    out["normal"] = u
    out["rgba"] = np.concatenate([rgb, (mask * f32(255)).astype(np.uint8)[..., None]], -1)
    return out


def general_scenes():
    """Three perspective scenes of tests/test_render_gpu.py at S = 64: name -> (V (V, 3) fp64, F, cameras)."""
    import test_render_gpu as TR
    from actionmesh_amd import render as R
    V, F = TR.icosphere(2, 0.9)
    rng = np.random.default_rng(3)
    V = V * rng.uniform(0.8, 1.15, size=(len(V), 1)) + rng.normal(0, 0.03, size=V.shape)
    views = [R.uniform_cameras(distance=3.0)[t] for t in R.VISUALIZER_CAMERAS]
    two_behind = np.array([(-0.5, -0.5, -3.0), (0.6, -0.4, -3.0), (0.0, 0.3, 0.0)])
    one_behind = np.array([(-0.5, -0.5, 0.0), (0.6, -0.4, 0.0), (0.0, 0.3, -3.0)])
    quad = np.array([(-3.0, -3.05, 0.5), (3.0, -3.05, 0.5), (3.0, 2.95, 0.5), (-3.0, 2.95, 0.5)])
    straddle = (np.concatenate([quad, two_behind, one_behind]), np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [7, 8, 9]]), [TR.cam()])
    fill = (np.array([(-3.0, -3.05, 0.0), (3.0, -3.05, 0.0), (3.0, 2.95, 0.0), (-3.0, 2.95, 0.0)]), np.array([[0, 1, 2], [0, 2, 3]]),
            [TR.cam()])
    return {"jittered_icosphere": (V, F, views), "straddlers": straddle, "frame_filling_quad": fill}


def render_batch(V, F, cams, S, fault=None, normals=True):
    """One frame under every camera, stacked as HipRenderer.render_normals returns it: (1, C, ...)."""
    X = np.asarray(V, dtype=np.float64).astype(f32)
    per_image = int(queued(project(X, cams[0]), F, 2 * S).sum()) if fault == "one_stride" else 0
    imgs = [render(X, F, cam, S, fault, normals, queue_base=c * per_image) for c, cam in enumerate(cams)]
    return {k: np.stack([im[k] for im in imgs])[None] for k in imgs[0]}
