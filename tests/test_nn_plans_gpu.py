"""am_nn_search at the launch plan the older shape tests never select: four queries per thread (nn_search_kernel<T, 4>, both
precisions) - the clamp of a thread's extra lanes to query Q - 1, the guarded store, ragged point tiles, and a batch that reaches the
threshold by its size rather than by the query count.  Every comparison is exact: fp64 and fp32 brute force in the kernel's
summation order (contraction is off in the kernel)."""
import numpy as np
import pytest
import torch

from actionmesh_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"

NN_THREADS, NN_TILE = 256, 512          # csrc/am_points.h


def nn_plan(P, Q, batch):
    """mirrors nn_plan() of csrc/am_pointcloud.hip: (queries per thread, query blocks, point splits)"""
    cdiv = lambda a, b: -(-a // b)
    qpt = 4 if Q * batch >= 4 * NN_THREADS * 512 else 1
    qblocks = cdiv(Q, NN_THREADS * qpt)
    blocks = qblocks * batch
    want = 1 if blocks >= 512 else cdiv(512, blocks)
    want = max(1, min(want, cdiv(P, 4 * NN_TILE)))
    chunk = cdiv(cdiv(P, want), NN_TILE) * NN_TILE
    return qpt, qblocks, cdiv(P, chunk)


def brute(q, p, dtype):
    """(index of the first minimum, that d2) of ((dx*dx) + (dy*dy)) + dz*dz evaluated in `dtype`; q (B, n, 3), p (B, P, 3) fp32"""
    q, p = q.astype(dtype), p.astype(dtype)
    d = q[:, :, None, :] - p[:, None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d2.dtype == dtype
    i = d2.argmin(axis=2)                                  # numpy: the first minimum, like the kernel's strict <
    return i, np.take_along_axis(d2, i[..., None], 2)[..., 0]


# (P, Q, B): Q % 1024 = 3 over three point tiles with a ragged last one; a batch of 3 that reaches the threshold, Q % 4 = 3; one full
# and one almost empty query block per batch entry
SHAPES = [(1100, 524_291, 1), (700, 174_763, 3), (5, 1025, 512)]


@pytest.mark.parametrize("shared", [False, True], ids=["batched-cloud", "shared-cloud"])
@pytest.mark.parametrize("P,Q,B", SHAPES)
def test_nn_four_queries_per_thread(P, Q, B, shared):
    qpt, qblocks, nsplit = nn_plan(P, Q, B)
    assert (qpt, nsplit) == (4, 1), "the shape must select four queries per thread in one split"
    assert Q % 4 != 0 and qblocks * NN_THREADS * 4 > Q > (qblocks - 1) * NN_THREADS * 4       # the last block clamps and guards
    g = torch.Generator().manual_seed(P * 31 + Q)
    pts = torch.randn((1 if shared else B, P, 3), generator=g)
    qry = torch.randn((B, Q, 3), generator=g)
    dup = 3 if P > 10 else 1
    pts[:, P - 1] = pts[:, dup]             # an exact duplicate: the lower index must win
    qry[:, 0] = pts[:, dup]                 # a coincident query, first of every batch entry ...
    qry[:, Q - 1] = pts[:, dup]             # ... and the very last one, which the clamped lanes repeat
    pts_b = pts.expand(B, P, 3)
    operand = pts[0].contiguous() if shared else pts
    # the first 8 and last 8 queries of every batch entry plus a stride over the rest, below 4e6 pairs for the CPU
    step = max(1, -(-(P * Q * B) // 3_900_000))
    sub = np.unique(np.concatenate([np.arange(8), np.arange(0, Q, step), np.arange(Q - 8, Q)]))
    assert P * len(sub) * B <= 4_000_000
    for precise, dtype in ((True, np.float64), (False, np.float32)):
        idx, d2 = ops.nearest_neighbors(operand.to(DEV), qry.to(DEV), precise=precise)
        torch.cuda.synchronize()
        assert idx.shape == (B, Q) and d2.dtype == (torch.float64 if precise else torch.float32)
        idx, d2 = idx.cpu().long(), d2.cpu()
        assert int(idx.min()) >= 0 and int(idx.max()) < P
        # all queries: the reported d2 is the distance to the reported index, bitwise
        t = torch.float64 if precise else torch.float32
        diff = qry.to(t) - torch.gather(pts_b.to(t), 1, idx[..., None].expand(-1, -1, 3))
        sq = diff * diff
        assert torch.equal((sq[..., 0] + sq[..., 1]) + sq[..., 2], d2), f"precise={precise}: d2 is not the distance to the index"
        # the subsample: index and d2 equal the brute force of the same precision and operation order, bit for bit
        ri, rd = brute(qry[:, sub].numpy(), pts_b.numpy(), dtype)
        assert np.array_equal(idx[:, sub].numpy(), ri), f"precise={precise}: index differs from the brute force"
        assert np.array_equal(d2[:, sub].numpy().view(np.uint8), rd.view(np.uint8)), f"precise={precise}: d2 differs from the brute force"
        assert (idx[:, 0] == dup).all() and (d2[:, 0] == 0).all() and (idx[:, Q - 1] == dup).all() and (d2[:, Q - 1] == 0).all()
