"""Farthest-point sampling, the parts that need no GPU (seam S7).

* `fps_restatement`: the yardstick of this module AND of tests/test_fps_gpu.py - the contract of `am_fps`
  (include/actionmesh_amd.h) restated in numpy fp32, one rounding per product and per sum, `np.argmax` = first maximum.
* C-ABI argument validation without a device; no CPU path in `ops`.
* The mirrored names of `actionmesh_amd.pointcloud_sampling` have the reference's signatures: recorded in
  tests/golden/pointcloud_sampling_signatures.json, and re-read from the live reference module where the checkout is present.
* The orchestration (`sample_pc`, `sample_pc_grouped`: identity / RANDOM / pre-sampling / chunks / grouping) against the
  reference's OWN functions.  The reference module imports PyTorch3D and fpsample, which do not exist here: test-local stub modules
  whose FPS is the restatement stand in for them (sys.modules entries that monkeypatch removes again), and the same restatement
  replaces the mirror's kernel call, so that what is compared is everything around the FPS.  B = 1 where the reference's CPU
  branch demands it.
* `install_into` on a stand-in module object (the triposg package is not installed where these tests run); `dropin.install`
  keeps its parameters and defaults and gains `pointcloud=False`.
"""
import ctypes
import importlib
import inspect
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from actionmesh_amd import _lib, cli, dropin, ops
from actionmesh_amd import pointcloud_sampling as S

REF = "/root/reference"
HAVE_REF = os.path.isdir(os.path.join(REF, "actionmesh"))
MIRRORED = ("sample_from_indices", "sample_pc", "sample_pc_grouped", "_farthest_point_sample", "_sample_fps")


def fps_restatement(points, n_samples, start=0, dist_dims=None):
    """Exact greedy FPS of one cloud (N, D): (indices int64 (K,), out_dist fp32 (K,)).  fp32 throughout; numpy rounds every product
    and every sum on its own (two ufunc calls, no fma); the sum runs left to right over the first dist_dims channels."""
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float32))
    dd = p.shape[1] if dist_dims is None else dist_dims
    md = np.full(p.shape[0], np.inf, dtype=np.float32)
    idx, dist = np.empty(n_samples, np.int64), np.empty(n_samples, np.float32)
    cur = int(start)
    for k in range(n_samples):
        idx[k], dist[k] = cur, md[cur]
        d = p[:, :dd] - p[cur, :dd]
        acc = d[:, 0] * d[:, 0]
        for c in range(1, dd):
            acc = acc + d[:, c] * d[:, c]
        md = np.minimum(md, acc)
        cur = int(np.argmax(md))
    return idx, dist


def fps_restatement_batch(points, n_samples, start_idx=None):
    """torch (B, N, D) -> int64 (B, K): the restatement behind the signature of pointcloud_sampling._fps_core."""
    pts = points.detach().float().cpu().numpy()
    starts = [0] * len(pts) if start_idx is None else [int(s) for s in start_idx]
    out = np.stack([fps_restatement(p, n_samples, s)[0] for p, s in zip(pts, starts)])
    return torch.from_numpy(out).to(points.device)


# ---- the restatement itself ---------------------------------------------------------------------------------------------------
def test_restatement_against_an_independent_loop():
    """The yardstick against a scalar Python loop that shares no code with it (np.float32 scalars: one rounding per operation)."""
    rng = np.random.default_rng(0)
    p = rng.standard_normal((60, 3)).astype(np.float32)
    p[40:50] = p[0:10]                                  # duplicates: ties
    idx, dist = fps_restatement(p, 60, start=7)
    md = [np.float32(np.inf)] * 60
    cur = 7
    for k in range(60):
        assert idx[k] == cur and (dist[k] == md[cur])
        for i in range(60):
            d = [np.float32(p[i, c] - p[cur, c]) for c in range(3)]
            d2 = np.float32(np.float32(np.float32(d[0] * d[0]) + np.float32(d[1] * d[1])) + np.float32(d[2] * d[2]))
            md[i] = min(md[i], d2)
        best = max(md)
        cur = md.index(best)                            # first maximum
    assert np.all(dist[2:] <= dist[1:-1])
    assert dist[50] == 0 and np.all(idx[50:] == 0)      # 50 distinct points: from there on index 0 repeats


# ---- 1. argument validation ---------------------------------------------------------------------------------------------------
def _args(**kw):
    a = _lib.AmFpsArgs()
    # pointers that are never dereferenced: every case below must be refused before anything touches a device
    a.points, a.out_index = 0x1000, 0x1000
    a.dtype, a.batch, a.n_points, a.dims, a.dist_dims = _lib.FPS_F32, 1, 16, 3, 3
    a.batch_stride, a.point_stride, a.n_samples = 48, 3, 4
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw, word", [
    (dict(n_points=0), b"empty"), (dict(batch=0), b"empty"), (dict(n_samples=0), b"n_samples"), (dict(n_samples=17), b"n_samples"),
    (dict(dims=0), b"dims"), (dict(dims=9, point_stride=9), b"dims"), (dict(dist_dims=4), b"dist_dims"), (dict(dist_dims=0), b"dist_dims"),
    (dict(dtype=7), b"dtype"), (dict(point_stride=2), b"point_stride"), (dict(points=None), b"null"), (dict(out_index=None), b"null"),
    (dict(threads=100), b"threads"), (dict(n_points=1 << 31, n_samples=4), b"32-bit"), (dict(n_points=100000, batch_stride=300000), b"workspace"),
])
def test_fps_argument_validation_without_gpu(kw, word):
    lib = _lib.lib()
    assert lib.am_fps(ctypes.byref(_args(**kw)), None) != 0
    assert word in lib.am_last_error(), lib.am_last_error()


def test_fps_null_arguments_and_workspace_size():
    lib = _lib.lib()
    assert lib.am_fps(None, None) != 0 and b"null" in lib.am_last_error()
    assert lib.am_fps_workspace_bytes(8192, 16, 3) == 0              # the resident form needs none
    assert lib.am_fps_workspace_bytes(8193, 2, 3) == 4 * 8196 * 2 * 4   # the streaming form: md + 3 channels, fp32, points padded to 4
    assert lib.am_fps_workspace_bytes(70001, 1, 6) == 4 * 70004 * 7


def test_ops_fps_has_no_cpu_path():
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.farthest_point_sample(torch.zeros(1, 16, 3), 4)
    with pytest.raises(RuntimeError, match="no CPU path"):        # and so has the mirror: nothing is computed in torch instead
        S.sample_pc(torch.zeros(1, 16, 3), 4, "fps", fps_random=False)


# ---- 2. signatures ------------------------------------------------------------------------------------------------------------
def _record(fn):
    return [[n, int(p.kind), None if p.default is inspect.Parameter.empty else repr(p.default)]
            for n, p in inspect.signature(fn).parameters.items()]


def _recorded(golden_dir):
    with open(os.path.join(golden_dir, "pointcloud_sampling_signatures.json")) as f:
        return json.load(f)


def test_mirrored_signatures_equal_the_recorded_references(golden_dir):
    rec = _recorded(golden_dir)
    assert set(MIRRORED) <= set(rec)
    for name in MIRRORED:
        assert _record(getattr(S, name)) == rec[name], name
    assert [(m.name, m.value) for m in S.SamplingType] == [tuple(m) for m in rec["SamplingType"]]
    assert issubclass(S.SamplingType, str)
    # the two PyTorch3D names, as the reference calls them (pointcloud_sampling.py:59-64, 116; triposg.py:151)
    assert list(inspect.signature(S.masked_gather).parameters) == ["points", "idx"]
    sig = inspect.signature(S.sample_farthest_points).parameters
    assert list(sig) == ["points", "lengths", "K", "random_start_point"] and sig["random_start_point"].default is False


@pytest.fixture
def reference_sampling(monkeypatch):
    """The reference's own pointcloud_sampling module, imported under stub `pytorch3d.ops`, `pytorch3d.ops.utils` and `fpsample`
    whose FPS is the restatement; every sys.modules entry made here is removed again."""
    if not HAVE_REF:
        pytest.skip("reference not present")

    def sample_farthest_points(points, lengths=None, K=50, random_start_point=False):
        assert lengths is None and not random_start_point
        idx = fps_restatement_batch(points, K)
        return S.masked_gather(points, idx), idx

    def bucket_fps_kdline_sampling(pts, n_samples, level, start_idx=None):
        assert start_idx == 0 and level in (5, 7)
        return fps_restatement(pts.numpy(), n_samples, 0)[0]

    p3d, p3d_ops, p3d_utils = types.ModuleType("pytorch3d"), types.ModuleType("pytorch3d.ops"), types.ModuleType("pytorch3d.ops.utils")
    p3d.__path__, p3d_ops.__path__ = [], []
    p3d_ops.sample_farthest_points, p3d_utils.masked_gather = sample_farthest_points, S.masked_gather
    p3d.ops, p3d_ops.utils = p3d_ops, p3d_utils
    fps_pkg, fps_mod = types.ModuleType("fpsample"), types.ModuleType("fpsample.fpsample")
    fps_mod.bucket_fps_kdline_sampling = bucket_fps_kdline_sampling
    fps_pkg.fpsample = fps_mod
    for name, mod in (("pytorch3d", p3d), ("pytorch3d.ops", p3d_ops), ("pytorch3d.ops.utils", p3d_utils), ("fpsample", fps_pkg),
                      ("fpsample.fpsample", fps_mod)):
        monkeypatch.setitem(sys.modules, name, mod)
    before = set(sys.modules)
    monkeypatch.syspath_prepend(REF)
    try:
        yield importlib.import_module("actionmesh.model.utils.pointcloud_sampling")
    finally:
        for name in set(sys.modules) - before:
            if name == "actionmesh" or name.startswith("actionmesh."):
                del sys.modules[name]


def test_recorded_signatures_are_the_references(reference_sampling, golden_dir):
    rec = _recorded(golden_dir)
    for name in MIRRORED:
        assert _record(getattr(reference_sampling, name)) == rec[name], name
    assert [[m.name, m.value] for m in reference_sampling.SamplingType] == rec["SamplingType"]


# ---- 3. orchestration against the reference's own functions ---------------------------------------------------------------------
def _cloud(B, N, D, seed):
    return torch.randn((B, N, D), generator=torch.Generator().manual_seed(seed))


ORCHESTRATION = [
    # (B, N, D, n_samples, keywords)
    (2, 40, 6, 40, dict(sampling_type="fps")),                                              # identity: N <= n_samples
    (2, 30, 3, 64, dict(sampling_type="random")),                                           # identity
    (3, 500, 6, 64, dict(sampling_type="random")),                                          # RANDOM: the same randperm draws
    (1, 500, 6, 64, dict(sampling_type="fps", fps_random=False)),
    (1, 500, 6, 64, dict(sampling_type="fps_full", fps_random=False)),
    (1, 500, 6, 64, dict(sampling_type=None, fps_random=False)),                            # the enum member instead of its string
    (1, 900, 6, 64, dict(sampling_type="fps", fps_random=False, fps_max_points=300)),       # pre-sampling, then FPS
    (1, 900, 6, 64, dict(sampling_type="fps", fps_random=False, fps_max_points=32)),        # pre-sampling down to n_samples: no FPS left
    (1, 512, 6, 64, dict(sampling_type="fps", fps_random=False, fps_chunks=1)),
    (1, 512, 6, 64, dict(sampling_type="fps", fps_random=False, fps_chunks=2)),
    (1, 512, 6, 64, dict(sampling_type="fps_full", fps_random=False, fps_chunks=4)),
    (1, 510, 3, 64, dict(sampling_type="fps", fps_random=False, fps_chunks=4)),             # unequal chunks (128, 128, 128, 126): the loop
    (1, 900, 6, 64, dict(sampling_type="fps", fps_random=False, fps_max_points=400, fps_chunks=4)),
]


@pytest.mark.parametrize("B, N, D, n_samples, kw", ORCHESTRATION)
def test_sample_pc_matches_the_references_own(reference_sampling, monkeypatch, B, N, D, n_samples, kw):
    monkeypatch.setattr(S, "_fps_core", fps_restatement_batch)
    pts = _cloud(B, N, D, seed=N + D)
    kw_ref, kw_ours = dict(kw), dict(kw)
    if kw["sampling_type"] is None:
        kw_ref["sampling_type"], kw_ours["sampling_type"] = reference_sampling.SamplingType.FPS, S.SamplingType.FPS
    torch.manual_seed(11)
    want_p, want_i = reference_sampling.sample_pc(pts, n_samples, **kw_ref)
    torch.manual_seed(11)
    got_p, got_i = S.sample_pc(pts, n_samples, **kw_ours)
    assert got_i.dtype == want_i.dtype == torch.int64 and got_i.shape == want_i.shape
    assert torch.equal(got_i, want_i) and torch.equal(got_p, want_p)
    # both consumed the global generator alike: the next draw agrees too
    torch.manual_seed(11); reference_sampling.sample_pc(pts, n_samples, **kw_ref); a = torch.rand(1)
    torch.manual_seed(11); S.sample_pc(pts, n_samples, **kw_ours); b = torch.rand(1)
    assert torch.equal(a, b)


@pytest.mark.parametrize("kw", [dict(fps_random=False), dict(fps_random=False, fps_chunks=2), dict(sampling_type="random"),
                                dict(fps_random=False, fps_max_points=200)])
def test_sample_pc_grouped_matches_the_references_own(reference_sampling, monkeypatch, kw):
    monkeypatch.setattr(S, "_fps_core", fps_restatement_batch)
    T = 3
    pts = _cloud(1 * T, 400, 6, seed=5)                # B = 1, T = 3 frames
    torch.manual_seed(3)
    want_p, want_i = reference_sampling.sample_pc_grouped(pts, 32, T, **kw)
    torch.manual_seed(3)
    got_p, got_i = S.sample_pc_grouped(pts, 32, T, **kw)
    assert torch.equal(got_i, want_i) and torch.equal(got_p, want_p)
    assert torch.equal(got_i[0], got_i[1]) and torch.equal(got_i[0], got_i[2])


def test_random_start_and_chunk_folding(monkeypatch):
    """fps_random=True: one torch.randint(N, (B,)) per FPS call from the global generator; the folded chunks (one launch) draw chunk
    by chunk and give what independent per-chunk runs give."""
    seen = []

    def core(points, n_samples, start_idx=None):
        seen.append((tuple(points.shape), None if start_idx is None else start_idx.clone()))
        return fps_restatement_batch(points, n_samples, start_idx)
    monkeypatch.setattr(S, "_fps_core", core)
    pts = _cloud(2, 512, 6, seed=2)
    torch.manual_seed(9)
    _, idx = S.sample_pc(pts, 64, "fps", fps_random=True)
    torch.manual_seed(9)
    start = torch.randint(512, (2,))
    assert torch.equal(seen[0][1], start) and seen[0][0] == (2, 512, 3)
    assert torch.equal(idx, fps_restatement_batch(pts[..., :3], 64, start))
    # four chunks of 128 folded into ONE call of 8 clouds
    seen.clear()
    torch.manual_seed(9)
    got_p, got_i = S.sample_pc(pts, 64, "fps", fps_random=True, fps_chunks=4)
    assert len(seen) == 1 and seen[0][0] == (8, 128, 3)
    torch.manual_seed(9)
    parts = []
    for c in range(4):
        st = torch.randint(128, (2,))
        parts.append(fps_restatement_batch(pts[:, 128 * c:128 * (c + 1), :3], 16, st) + 128 * c)
    assert torch.equal(got_i, torch.cat(parts, dim=1))
    assert torch.equal(got_p, S.masked_gather(pts, got_i))


def test_masked_gather_and_sample_from_indices():
    pts = _cloud(2, 10, 4, seed=1)
    idx = torch.tensor([[3, -1, 0], [9, 9, -1]])
    out = S.masked_gather(pts, idx)
    assert torch.equal(out[0, 0], pts[0, 3]) and torch.equal(out[1, 1], pts[1, 9]) and not out[0, 1].any() and not out[1, 2].any()
    assert idx[0, 1] == -1                                   # the caller's indices are not written to
    out3 = S.masked_gather(pts, idx[:, None, :].expand(-1, 5, -1).contiguous())
    assert out3.shape == (2, 5, 3, 4) and torch.equal(out3[:, 2], out)
    assert torch.equal(S.sample_from_indices(pts, torch.tensor([[1, 2]])), pts[:, 1:3])      # (1, M) is shared by the batch
    with pytest.raises(ValueError):
        S.sample_from_indices(pts, torch.zeros((3, 2), dtype=torch.long))
    with pytest.raises(ValueError):
        S.sample_pc(pts, 6, "fps", fps_chunks=4)             # n_samples must divide into the chunks
    with pytest.raises(ValueError):
        S.sample_pc(pts, 4, "nearest")
    with pytest.raises(NotImplementedError):
        S.sample_farthest_points(pts, lengths=torch.tensor([10, 5]), K=2)


# ---- 4. the drop-in seam ------------------------------------------------------------------------------------------------------
def test_install_into_a_stand_in_module():
    """What actionmesh/external/triposg.py looks like after its guarded import failed (lines 17-23): only the flag, set to False."""
    mod = types.ModuleType("triposg_stand_in")
    mod._is_pytorch3d_available = False
    mod.masked_gather = "someone else's"
    registered = "pytorch3d" in sys.modules
    saved = S.install_into(mod)
    assert mod.sample_pc is S.sample_pc and mod.sample_pc_grouped is S.sample_pc_grouped and mod.masked_gather is S.masked_gather
    assert mod._is_pytorch3d_available is True
    assert ("pytorch3d" in sys.modules) == registered        # no stand-in pytorch3d: `import pytorch3d` keeps deciding as before
    S.uninstall_from(mod, saved)
    assert mod._is_pytorch3d_available is False and mod.masked_gather == "someone else's"
    assert not hasattr(mod, "sample_pc") and not hasattr(mod, "sample_pc_grouped")


def test_dropin_install_keeps_its_parameters_and_gains_pointcloud():
    params = inspect.signature(dropin.install).parameters
    assert [(n, p.default) for n, p in params.items()] == [
        ("attn_dtype", "bf16"), ("stage2", False), ("use_graph", None), ("stage2_cross_fp32", False), ("render", False),
        ("pointcloud", False)]


def test_cli_pointcloud_flag_defaults_to_off():
    ours, rest = cli.split_args(["--input", "a"])
    assert ours.pointcloud == "off" and rest == ["--input", "a"]
    ours, rest = cli.split_args(["--pointcloud", "hip", "--script", "video_and_3d_to_animated_mesh", "--", "--input", "a"])
    assert ours.pointcloud == "hip" and rest == ["--input", "a"]
    with pytest.raises(SystemExit):
        cli.split_args(["--pointcloud", "auto"])
