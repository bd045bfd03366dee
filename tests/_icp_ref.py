"""am_icp_step restated in numpy from the comment in include/actionmesh_amd.h, step by step and in its order: x in fp32, brute-force fp32
matching (first minimum, a NaN or infinite distance never wins), fp32 terms, fp64 sums, the fp64 chain rule and Adam, fp32 stores and
the best-so-far rule.  numpy rounds every operation on its own and fuses nothing, which is what the header asks for.  The sums are
np.sum's order, not the kernel's tree: tests compare them within the fp64 reordering bound, and everything after the sums can be fed
the device's own sums (`sums=`), after which the header promises the same bits."""
import numpy as np

f32, f64 = np.float32, np.float64
NO_NEIGHBOUR = 1


def dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def cross(u, v):
    return np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]], f64)


def rotation(prm, ri):
    """step 1 for one candidate: prm (12,) fp32, ri (9,) fp32 -> R (3, 3) fp32 and the Gram-Schmidt quantities (fp64)"""
    a1, a2 = prm[3:6].astype(f64), prm[6:9].astype(f64)
    l1 = np.sqrt(dot(a1, a1))
    n1 = f64(1e-12) if l1 < 1e-12 else l1
    b1 = a1 / n1
    d = dot(b1, a2)
    u = a2 - d * b1
    l2 = np.sqrt(dot(u, u))
    n2 = f64(1e-12) if l2 < 1e-12 else l2
    b2 = u / n2
    G = np.stack((b1, b2, cross(b1, b2)))
    Ri = ri.astype(f64).reshape(3, 3)
    R64 = np.empty((3, 3), f64)
    for a in range(3):
        for j in range(3):
            R64[a, j] = (Ri[a, 0] * G[0, j] + Ri[a, 1] * G[1, j]) + Ri[a, 2] * G[2, j]
    return R64.astype(f32), dict(a1=a1, a2=a2, b1=b1, b2=b2, n1=n1, n2=n2, d=d)


def transform(pred, R, T, s):
    """step 2: (P, 3) fp32 -> (P, 3) fp32"""
    q = [(s[a] * pred[:, a]).astype(f32) for a in range(3)]
    x = np.empty_like(pred)
    for j in range(3):
        x[:, j] = ((q[0] * R[0, j] + q[1] * R[1, j]) + q[2] * R[2, j]) + T[j]
    return x


def match(queries, points, block=2048):
    """step 3: for every query the lowest index of the smallest finite d2, or -1"""
    out = np.empty(len(queries), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, len(queries), block):
            q = queries[lo:lo + block]
            dx, dy, dz = (q[:, None, k] - points[None, :, k] for k in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == f32
            d2 = np.where(d2 < np.inf, d2, f32(np.inf))           # NaN and +inf never win
            idx = d2.argmin(1)                                    # first minimum
            out[lo:lo + block] = np.where(d2[np.arange(len(q)), idx] < np.inf, idx, -1)
    return out


def pair_terms(x, y, p):
    """step 4: the (n, 13) fp64 terms of n matched pairs"""
    r = x - y
    assert r.dtype == f32
    t = np.empty((len(x), 13), f64)
    t[:, 0] = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
    t[:, 1:4] = r
    for a in range(3):
        for j in range(3):
            t[:, 4 + 3 * a + j] = p[:, a] * r[:, j]               # fp32 product, widened by the store
    return t


def terms(pred, gt, prm, ri):
    """steps 1-4 for one candidate: R (fp32), [terms of direction 0, terms of direction 1], flag"""
    R, _ = rotation(prm, ri)
    x = transform(pred, R, prm[0:3], prm[9:12])
    with np.errstate(invalid="ignore"):
        n, m = match(x, gt), match(gt, x)
        k0, k1 = n >= 0, m >= 0
        t0 = pair_terms(x[k0], gt[n[k0]], pred[k0])
        t1 = pair_terms(x[m[k1]], gt[k1], pred[m[k1]])
    return R, [t0, t1], (0 if k0.all() and k1.all() else NO_NEIGHBOUR)


def sums_of(pred, gt, params, rot_init):
    """-> sums (B, 2, 13) fp64, abs_sums (B, 2, 13) = the sums of the terms' magnitudes (for error bounds), counts (B, 2), flag"""
    B = len(params)
    sums, mags, counts, flag = np.zeros((B, 2, 13), f64), np.zeros((B, 2, 13), f64), np.zeros((B, 2), np.int64), 0
    for b in range(B):
        _, t, fl = terms(pred, gt, params[b], rot_init[b])
        flag |= fl
        for d in range(2):
            sums[b, d], mags[b, d], counts[b, d] = t[d].sum(0), np.abs(t[d]).sum(0), len(t[d])
    return sums, mags, counts, flag


def gradient(sums_b, prm, ri, P, Q, B):
    """step 5 for one candidate: sums_b (2, 13) fp64 -> loss fp32, R fp32, g (12,) fp64"""
    R, fr = rotation(prm, ri)
    w0, w1, c2 = f64(1.0) / f64(P), f64(1.0) / f64(Q), f64(2.0) / f64(B)
    A = w0 * sums_b[0] + w1 * sums_b[1]
    s, Rw, Ri = prm[9:12].astype(f64), R.astype(f64), ri.astype(f64).reshape(3, 3)
    g = np.empty(12, f64)
    g[0:3] = c2 * A[1:4]
    M = (c2 * A[4:13]).reshape(3, 3)
    gR = s[:, None] * M
    for a in range(3):
        g[9 + a] = (M[a, 0] * Rw[a, 0] + M[a, 1] * Rw[a, 1]) + M[a, 2] * Rw[a, 2]
    gG = np.empty((3, 3), f64)
    for i in range(3):
        for j in range(3):
            gG[i, j] = (Ri[0, i] * gR[0, j] + Ri[1, i] * gR[1, j]) + Ri[2, i] * gR[2, j]
    g1, g2, g3 = gG[0].copy(), gG[1].copy(), gG[2].copy()
    g1 = g1 + cross(fr["b2"], g3)
    g2 = g2 + cross(g3, fr["b1"])
    t2 = dot(g2, fr["b2"])
    gu = (g2 - t2 * fr["b2"]) / fr["n2"]
    t1 = dot(gu, fr["b1"])
    g[6:9] = gu - t1 * fr["b1"]
    g1 = g1 - (fr["d"] * gu + t1 * fr["a2"])
    t0 = dot(g1, fr["b1"])
    g[3:6] = (g1 - t0 * fr["b1"]) / fr["n1"]
    return A[0].astype(f32), R, g


def jacobian(prm, ri, P, Q, B):
    """(13, 26): d [loss, g] / d sums of one candidate - step 5 is linear in the sums, so a bound on the sums' error becomes a bound on
    the loss's and the gradient's through |J|"""
    J = np.empty((13, 26), f64)
    for k in range(26):
        e = np.zeros(26, f64)
        e[k] = 1.0
        _, _, g = gradient(e.reshape(2, 13), prm, ri, P, Q, B)
        J[0, k] = (1.0 / P if k == 0 else 1.0 / Q if k == 13 else 0.0)       # the loss before its fp32 rounding
        J[1:, k] = g
    return J


def adam(prm, m, v, g, t, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8):
    """step 6: fp32 state and fp64 gradient (any shape) -> the new fp32 (params, m, v)"""
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t             # host doubles, as torch computes them
    beta1, beta2, eps, lr = f64(beta1), f64(beta2), f64(eps), f64(lr)
    m2 = beta1 * m.astype(f64) + (f64(1.0) - beta1) * g
    v2 = beta2 * v.astype(f64) + (f64(1.0) - beta2) * (g * g)
    denom = np.sqrt(v2) / np.sqrt(f64(bc2)) + eps
    p2 = prm.astype(f64) - (lr / f64(bc1)) * (m2 / denom)
    return p2.astype(f32), m2.astype(f32), v2.astype(f32)


class State:
    """the fields of ops.IcpState, in numpy"""

    def __init__(self, B):
        self.params = np.tile(np.array([0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 1, 1], f32), (B, 1))
        self.adam_m, self.adam_v = np.zeros((B, 12), f32), np.zeros((B, 12), f32)
        self.best = np.zeros(16, f32)
        self.best[15] = np.inf
        self.out_loss, self.out_rot = np.zeros(B, f32), np.zeros((B, 9), f32)
        self.out_sums, self.out_grad, self.out_flag = np.zeros((B, 2, 13), f64), np.zeros((B, 12), f64), 0

    def copy(self):
        o = State(len(self.params))
        for k, v in vars(self).items():
            setattr(o, k, v.copy() if isinstance(v, np.ndarray) else v)
        return o


def step(st, pred, gt, rot_init, t, lr=0.01, update=True, sums=None):
    """one am_icp_step on a State, in place; `sums`: (B, 2, 13) fp64 to use instead of this file's own (the device's)"""
    B, P, Q = len(st.params), len(pred), len(gt)
    rot_init = rot_init.reshape(B, 9)
    if sums is None:
        sums, _, _, flag = sums_of(pred, gt, st.params, rot_init)
        st.out_flag |= flag
    st.out_sums = np.array(sums, f64)
    for b in range(B):
        st.out_loss[b], R, st.out_grad[b] = gradient(st.out_sums[b], st.params[b], rot_init[b], P, Q, B)
        st.out_rot[b] = R.reshape(9)
    if update:
        st.params, st.adam_m, st.adam_v = adam(st.params, st.adam_m, st.adam_v, st.out_grad, t, lr=lr)
        # step 7: the smallest loss, accepted on < only in ascending index (a NaN never wins), against the stored best
        c, lc = -1, f32(np.inf)
        for b in range(B):
            if st.out_loss[b] < lc:
                c, lc = b, st.out_loss[b]
        if c >= 0 and lc < st.best[15]:
            st.best = np.concatenate((st.out_rot[c], st.params[c, 0:3], st.params[c, 9:12], [lc])).astype(f32)
    return st
