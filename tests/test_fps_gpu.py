"""Farthest-point sampling on the device (csrc/am_fps.hip through ops.farthest_point_sample and the mirrors of
actionmesh_amd/pointcloud_sampling.py).  The contract of include/actionmesh_amd.h has no tolerance: indices AND out_dist are
compared BIT FOR BIT with the numpy restatement of tests/test_fps_cpu.py, no case exempted.  out_dist is what catches an
fma-contracted distance (the indices of a random cloud survive one)."""
import numpy as np
import pytest
import torch

from actionmesh_amd import ops
from actionmesh_amd import pointcloud_sampling as S
from test_fps_cpu import fps_restatement          # the tests directory is on sys.path (pytest rootdir / conftest)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cloud(B, N, D, seed, dtype=torch.float32):
    return torch.randn((B, N, D), generator=torch.Generator().manual_seed(seed)).to(dtype)


def _check(points_dev, K, start=None, dist_dims=None, **kw):
    """Run the kernel on a device tensor (B, N, D) (any strides) and compare every cloud with the restatement; returns (idx, dist)."""
    idx, dist = ops.farthest_point_sample(points_dev, K, start_idx=start, dist_dims=dist_dims, return_dist=True, **kw)
    assert idx.dtype == torch.int32 and dist.dtype == torch.float32 and idx.shape == dist.shape == (points_dev.shape[0], K)
    host = points_dev.float().cpu().numpy()
    idx_h, dist_h = idx.cpu().numpy(), dist.cpu().numpy()
    for b in range(host.shape[0]):
        s = 0 if start is None else int(start[b])
        want_i, want_d = fps_restatement(host[b], K, s, dist_dims)
        bad = np.flatnonzero(idx_h[b] != want_i)
        assert bad.size == 0, f"cloud {b}: first index mismatch at step {bad[0]}: {idx_h[b][bad[0]]} != {want_i[bad[0]]} ({bad.size} of {K})"
        assert np.array_equal(dist_h[b].view(np.uint32), want_d.view(np.uint32)), f"cloud {b}: out_dist differs in bits"
    return idx_h, dist_h


def test_tiny_cloud_first():
    """The smallest launches: (1, 5, 5, D = 2) and a single point."""
    _check(_cloud(1, 5, 2, 0).to(DEV), 5)
    i, d = _check(_cloud(1, 1, 3, 1).to(DEV), 1)
    assert i.tolist() == [[0]] and np.isinf(d[0, 0])


@pytest.mark.parametrize("threads", [0, 256, 512, 1024])
def test_product_shape(threads):
    """(1, 8192, 2048, 3): what TripoSGVAE._sample_features asks for; every workgroup size the library carries."""
    _check(_cloud(1, 8192, 3, 2).to(DEV), 2048, threads=threads)


def test_batch_with_four_start_points():
    _check(_cloud(4, 8192, 3, 3).to(DEV), 2048, start=torch.tensor([0, 8191, 4096, 17]))


def test_strided_xyz_view_of_a_six_channel_cloud():
    x = _cloud(2, 8192, 6, 4).to(DEV)
    view = x[..., :3]
    assert not view.is_contiguous() and view.data_ptr() == x.data_ptr()
    i_view, d_view = _check(view, 2048)
    i_dd, d_dd = _check(x, 2048, dist_dims=3)          # the same thing said with dist_dims
    assert np.array_equal(i_view, i_dd) and np.array_equal(d_view.view(np.uint32), d_dd.view(np.uint32))


@pytest.mark.parametrize("threads", [0, 1024])
def test_six_channel_distance(threads):
    _check(_cloud(2, 8192, 6, 5).to(DEV), 2048, threads=threads)


@pytest.mark.parametrize("B, N, K, D, dd", [(3, 1000, 999, 3, 3), (2, 2048, 300, 8, 8), (2, 2049, 300, 4, 4), (1, 8192, 8192, 3, 3),
                                            (2, 700, 64, 5, 2), (1, 63, 63, 1, 1)])
def test_other_resident_shapes(B, N, K, D, dd):
    _check(_cloud(B, N, D, N + D).to(DEV), K, start=torch.arange(B) * 7 % N, dist_dims=dd)


@pytest.mark.parametrize("B, N, K, D, dd, dtype", [(1, 70001, 512, 3, 3, torch.float32), (2, 8193, 96, 6, 6, torch.float16),
                                                   (2, 9000, 96, 6, 3, torch.bfloat16)])
def test_streaming_form(B, N, K, D, dd, dtype):
    """N past the resident limit (8192): md in the workspace, the cloud re-read every step."""
    _check(_cloud(B, N, D, N, dtype).to(DEV), K, start=torch.arange(B) * 4099 % N, dist_dims=dd)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_16_bit_inputs_at_the_product_shape(dtype):
    """Converted to fp32 exactly, then the same arithmetic.  16-bit coordinates collide far more often than fp32 ones: ties."""
    _check(_cloud(1, 8192, 3, 6, dtype).to(DEV), 2048)


def _lattice_with_duplicates():
    g = torch.arange(8, dtype=torch.float32)
    lat = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), dim=-1).reshape(-1, 3)            # 512 points, ties everywhere
    perm = torch.randperm(512, generator=torch.Generator().manual_seed(7))
    return torch.cat([lat, lat[perm[:100]]])[None]                                                # + 100 duplicates


def test_ties_lattice_with_duplicates():
    """K larger than the number of distinct points: once every point coincides with a chosen one the lowest-index rule returns
    index 0 again, with out_dist 0."""
    pts = _lattice_with_duplicates()
    i, d = _check(pts.to(DEV), 612, start=torch.tensor([5]))
    assert np.all(d[0, 512:] == 0) and np.all(i[0, 512:] == 0) and np.all(d[0, 1:512] > 0)
    assert len(set(i[0, :512].tolist())) == 512


def test_cloud_of_identical_points():
    pts = torch.full((2, 300, 3), 1.25)
    i, d = _check(pts.to(DEV), 40, start=torch.tensor([0, 123]))
    assert i[0].tolist() == [0] * 40 and i[1].tolist() == [123] + [0] * 39
    assert np.isinf(d[:, 0]).all() and np.all(d[:, 1:] == 0)


def test_properties_that_do_not_need_the_restatement():
    pts = _cloud(1, 8192, 3, 8)
    idx, dist = ops.farthest_point_sample(pts.to(DEV), 2048, return_dist=True)
    idx, dist = idx[0].cpu().long(), dist[0].cpu()
    assert int(idx.min()) >= 0 and int(idx.max()) < 8192
    assert torch.all(dist[1:] > 0) and idx.unique().numel() == 2048                  # distinct while out_dist > 0
    assert torch.isinf(dist[0]) and torch.all(dist[2:] <= dist[1:-1])                # non-increasing from k = 1 on
    chosen = pts[0, idx].double()
    d2 = torch.cdist(chosen, chosen).pow(2)
    d2.fill_diagonal_(float("inf"))
    # the greedy invariant: no two chosen points are closer than the last selection distance.  The kernel's fp32 d2 carries a few
    # roundings of 6e-8 relative each against the fp64 value here: 1e-5 covers them with room to spare
    assert float(d2.min()) >= float(dist[-1]) * (1 - 1e-5)


def test_non_finite_inputs_terminate_in_range():
    """Nothing is promised for NaN / inf coordinates except termination with indices inside [0, N)."""
    for n in (4000, 9000):                                                             # resident and streaming form
        pts = _cloud(1, n, 3, 9)
        pts[0, 5, 0], pts[0, 77, 1], pts[0, 300, 2] = float("nan"), float("inf"), float("-inf")
        with pytest.raises(ValueError, match="non-finite"):
            ops.farthest_point_sample(pts.to(DEV), 8)
        idx = ops.farthest_point_sample(pts.to(DEV), 256, check=False).cpu()
        assert int(idx.min()) >= 0 and int(idx.max()) < n


def test_wrapper_arguments():
    pts = _cloud(2, 64, 3, 10).to(DEV)
    with pytest.raises(ValueError, match="start_idx"):
        ops.farthest_point_sample(pts, 4, start_idx=torch.tensor([0, 64]))
    with pytest.raises(ValueError, match="n_samples"):
        ops.farthest_point_sample(pts, 65)
    with pytest.raises(ValueError, match="contiguous"):
        ops.farthest_point_sample(torch.zeros((2, 64, 6), device=DEV)[..., ::2], 2)
    flat = ops.farthest_point_sample(pts[0], 8, start_idx=3)                            # (N, D) in, (K,) out
    assert flat.shape == (8,) and torch.equal(flat, ops.farthest_point_sample(pts, 8, start_idx=torch.tensor([3, 3]))[0])


# ---- the mirrors on the device ------------------------------------------------------------------------------------------------
def _gather(points, idx):
    return torch.stack([p[i] for p, i in zip(points, idx)])


def test_sample_pc_fps_equals_gather_by_restatement():
    pts = _cloud(2, 3000, 6, 11)
    got_p, got_i = S.sample_pc(pts.to(DEV), 256, "fps", fps_random=False)
    want_i = torch.from_numpy(np.stack([fps_restatement(p[:, :3].numpy(), 256)[0] for p in pts]))
    assert got_i.dtype == torch.int64 and torch.equal(got_i.cpu(), want_i) and torch.equal(got_p.cpu(), _gather(pts, want_i))
    got_p, got_i = S.sample_pc(pts.to(DEV), 256, "fps_full", fps_random=False)
    want_i = torch.from_numpy(np.stack([fps_restatement(p.numpy(), 256)[0] for p in pts]))
    assert torch.equal(got_i.cpu(), want_i) and torch.equal(got_p.cpu(), _gather(pts, want_i))


def test_sample_pc_random_start_follows_the_global_generator():
    pts = _cloud(3, 2000, 3, 12)
    torch.manual_seed(21)
    _, got_i = S.sample_pc(pts.to(DEV), 128, "fps", fps_random=True)
    torch.manual_seed(21)
    start = torch.randint(2000, (3,))
    want_i = torch.from_numpy(np.stack([fps_restatement(p.numpy(), 128, int(s))[0] for p, s in zip(pts, start)]))
    assert torch.equal(got_i.cpu(), want_i) and torch.equal(got_i[:, 0].cpu(), start)


def test_sample_pc_chunks_equal_independent_runs():
    pts = _cloud(2, 4096, 6, 13)
    got_p, got_i = S.sample_pc(pts.to(DEV), 256, "fps", fps_random=False, fps_chunks=4)
    parts = [torch.from_numpy(np.stack([fps_restatement(p[1024 * c:1024 * (c + 1), :3].numpy(), 64)[0] for p in pts])) + 1024 * c
             for c in range(4)]
    want_i = torch.cat(parts, dim=1)
    assert torch.equal(got_i.cpu(), want_i) and torch.equal(got_p.cpu(), _gather(pts, want_i))
    # unequal chunks (4094 = 1024 + 1024 + 1024 + 1022) go chunk by chunk
    _, got_u = S.sample_pc(pts[:, :4094].to(DEV), 256, "fps", fps_random=False, fps_chunks=4)
    want_u = torch.cat([torch.from_numpy(np.stack([fps_restatement(c[:, :3].numpy(), 64)[0] for c in chunk])) + 1023 * k
                        for k, chunk in enumerate(pts[:, :4094].chunk(4, dim=1))], dim=1)
    assert torch.equal(got_u.cpu(), want_u)


def test_sample_pc_grouped_repeats_frame_zero():
    T = 3
    pts = _cloud(2 * T, 1500, 3, 14)
    got_p, got_i = S.sample_pc_grouped(pts.to(DEV), 100, T, fps_random=False)
    want = [torch.from_numpy(fps_restatement(pts[b * T].numpy(), 100)[0]) for b in range(2)]
    want_i = torch.stack([want[f // T] for f in range(2 * T)])
    assert torch.equal(got_i.cpu(), want_i) and torch.equal(got_p.cpu(), _gather(pts, want_i))


def test_triposg_sample_features_recipe_end_to_end():
    """TripoSGVAE._sample_features (triposg.py:128-151) on a stand-in module served by install_into: rng choice of 4 * 2048 from a
    20 480 x 6 fp16 surface, FPS on xyz with a random start, gather of all six channels."""
    import types
    mod = types.ModuleType("triposg_stand_in")
    S.install_into(mod)
    num_tokens, seed = 2048, 0
    x = _cloud(1, 20480, 6, 15, torch.float16)
    indices = np.random.default_rng(seed).choice(x.shape[1], num_tokens * 4, replace=num_tokens * 4 > x.shape[1])
    selected_host = x[:, indices]
    selected = selected_host.to(DEV)
    torch.manual_seed(33)
    _, sampled_indices = mod.sample_pc(points=selected[..., :3], n_samples=num_tokens, sampling_type="fps", fps_random=True)
    out = mod.masked_gather(selected, sampled_indices)
    torch.manual_seed(33)
    start = int(torch.randint(8192, (1,)))
    want_i = torch.from_numpy(fps_restatement(selected_host[0, :, :3].float().numpy(), num_tokens, start)[0])
    assert out.shape == (1, 2048, 6) and out.dtype == torch.float16
    assert torch.equal(sampled_indices.cpu()[0], want_i) and torch.equal(out.cpu()[0], selected_host[0, want_i])
