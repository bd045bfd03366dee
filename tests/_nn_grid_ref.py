"""numpy restatement of the grid nearest-neighbour search as include/actionmesh_amd.h writes it (am_nn_grid ...): the build and the
search operation by operation, fp32 cell arithmetic, distances in fp32 or fp64.  Slow (a Python loop per query and ring): for the
small clouds of the tests.  brute() is the am_nn_search contract: the minimum over ALL points, ties to the lowest index."""
import numpy as np

F32 = np.float32


def fmap(a):
    """order-preserving map float32 -> uint32 (-0 below +0)"""
    u = np.ascontiguousarray(a, dtype=F32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def funmap(u):
    u = np.asarray(u, dtype=np.uint32)
    return np.where(u >> 31 != 0, u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32).view(F32)


def default_cells(n_points):
    g = 1
    while g ** 3 < 2 * n_points:
        g += 1
    return min(g, 128)


def cell_axes(p, frame, G):
    """the header's clamped cell (step 2 of the search), per axis, of every row of finite coordinates p (n, 3): (n, 3) int64"""
    c = np.zeros(p.shape, dtype=np.int64)
    with np.errstate(all="ignore"):
        for k in range(3):
            inv = frame[4 + k]
            if inv != 0:
                t = ((p[:, k] - frame[k]).astype(F32) * inv).astype(F32)
                mid = (t >= 0) & (t < F32(G))
                c[t >= F32(G), k] = G - 1
                c[mid, k] = np.floor(t[mid]).astype(np.int64)
    return c


def cells_of(points, frame, G):
    """the header's cell of every point: (cell (P,) int32, per-axis cells (P, 3), finite mask)"""
    p = np.ascontiguousarray(points, dtype=F32)
    finite = np.isfinite(p).all(axis=1)
    c = np.zeros(p.shape, dtype=np.int64)
    c[finite] = cell_axes(p[finite], frame, G)
    cell = (c[:, 2] * G + c[:, 1]) * G + c[:, 0]
    cell[~finite] = G ** 3
    return cell.astype(np.int32), c, finite


def build(points, G):
    """one cloud (P, 3) -> dict of the grid's arrays with the header's shapes and dtypes"""
    p = np.ascontiguousarray(points, dtype=F32)
    P = len(p)
    finite = np.isfinite(p).all(axis=1)
    frame = np.zeros(8, dtype=F32)
    if finite.any():
        keys = fmap(p[finite])
        lo, hi = funmap(keys.min(axis=0)), funmap(keys.max(axis=0))
        with np.errstate(all="ignore"):
            ext = (hi - lo).astype(F32)
            q = (F32(G) / ext).astype(F32)
        frame[:3] = lo
        frame[4:7] = np.where((ext == 0) | ~np.isfinite(q), F32(0), q)
    cell, c, _ = cells_of(p, frame, G)
    order = np.argsort(cell, kind="stable").astype(np.int32)
    cell_start = np.searchsorted(cell[order], np.arange(G ** 3 + 2), side="left").astype(np.int32)
    srt = np.empty((P, 4), dtype=F32)
    srt[:, :3] = p[order]
    srt[:, 3] = order.view(F32)
    mn = np.full((3, G), 0xFFFFFFFF, dtype=np.uint32)
    mx = np.zeros((3, G), dtype=np.uint32)
    keys = fmap(p)
    for k in range(3):
        np.minimum.at(mn[k], c[finite, k], keys[finite, k])
        np.maximum.at(mx[k], c[finite, k], keys[finite, k])
    smin = np.minimum.accumulate(mn[:, ::-1], axis=1)[:, ::-1]
    pmax = np.maximum.accumulate(mx, axis=1)
    slabs = np.empty((2, 3, G), dtype=F32)
    slabs[0] = np.where(smin == 0xFFFFFFFF, F32(np.inf), funmap(smin))
    slabs[1] = np.where(pmax == 0, F32(-np.inf), funmap(pmax))
    return {"cells": G, "n_points": P, "frame": frame, "cell": cell, "order": order, "cell_start": cell_start, "sorted": srt, "slabs": slabs}


def search(grid, queries, dtype=np.float64, count=None):
    """the header's ring walk for every query (Q, 3): (index int32, d2 dtype).  `count`: a list that receives the number of
    candidate points each query evaluated."""
    G, P = grid["cells"], grid["n_points"]
    frame, cs, slabs = grid["frame"], grid["cell_start"].astype(np.int64), grid["slabs"]
    pts = grid["sorted"][:, :3].astype(dtype)
    pidx = np.ascontiguousarray(grid["sorted"][:, 3]).view(np.int32)
    qs = np.ascontiguousarray(queries, dtype=F32)
    out_i = np.full(len(qs), -1, dtype=np.int32)
    out_d = np.full(len(qs), np.inf, dtype=dtype)
    inf = dtype(np.inf)
    for n, qf in enumerate(qs):
        evaluated = 0
        if np.isfinite(qf).all():
            c = [int(v) for v in cell_axes(qf[None, :], frame, G)[0]]
            q = qf.astype(dtype)
            best, bi = inf, -1
            for r in range(G):
                x0, x1 = max(c[0] - r, 0), min(c[0] + r, G - 1)
                ranges = []
                for z in range(max(c[2] - r, 0), min(c[2] + r, G - 1) + 1):
                    for y in range(max(c[1] - r, 0), min(c[1] + r, G - 1) + 1):
                        row = (z * G + y) * G
                        if z in (c[2] - r, c[2] + r) or y in (c[1] - r, c[1] + r):
                            ranges.append((row + x0, row + x1))
                        else:
                            if c[0] - r >= 0:
                                ranges.append((row + c[0] - r, row + c[0] - r))
                            if c[0] + r < G:
                                ranges.append((row + c[0] + r, row + c[0] + r))
                pos = [np.arange(cs[a], cs[b + 1]) for a, b in ranges if cs[b + 1] > cs[a]]
                if pos:
                    pos = np.concatenate(pos)
                    evaluated += len(pos)
                    with np.errstate(all="ignore"):
                        d = q[None, :] - pts[pos]
                        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                    ok = d2 <= best                      # NaN never
                    if ok.any():
                        m = d2[ok].min()
                        cand = pidx[pos[ok]][d2[ok] == m].min()
                        if m < best or (m == best and cand < bi):
                            best, bi = m, int(cand)
                gmin = inf
                with np.errstate(all="ignore"):
                    for k in range(3):
                        hi, lo = c[k] + r + 1, c[k] - r - 1
                        if hi < G:
                            gmin = min(gmin, dtype(slabs[0, k, hi]) - q[k])
                        if lo >= 0:
                            gmin = min(gmin, q[k] - dtype(slabs[1, k, lo]))
                    if not gmin < inf or best < gmin * gmin:
                        break
            if bi >= 0:
                out_i[n], out_d[n] = bi, best
        if count is not None:
            count.append(evaluated)
    return out_i, out_d


def brute(points, queries, dtype=np.float64):
    """am_nn_search: (index int32, d2 dtype) over all points; strict '<' from the first point on, -1 / +inf when nothing is finite"""
    p, q = np.asarray(points, dtype=F32).astype(dtype), np.asarray(queries, dtype=F32).astype(dtype)
    with np.errstate(all="ignore"):
        d = q[:, None, :] - p[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    d2 = np.where(np.isnan(d2), np.inf, d2).astype(dtype)
    idx = d2.argmin(axis=1).astype(np.int32)                 # first minimum
    best = d2[np.arange(len(q)), idx]
    idx[~(best < np.inf)] = -1
    return idx, best
