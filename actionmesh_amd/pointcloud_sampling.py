"""Point-cloud sampling behind the reference's own interface (INTEGRATION seam S7).

The reference's `actionmesh/model/utils/pointcloud_sampling.py` imports `pytorch3d.ops.sample_farthest_points` and
`pytorch3d.ops.utils.masked_gather` at module level and, off CUDA, `fpsample`; none of the three exists for ROCm, so where this
package runs `actionmesh.external.triposg` finds no `sample_pc` and `TripoSGVAE.__init__` raises ImportError (triposg.py:17-23,
106-110).  This module restates that file's public names with identical signatures and control flow - `SamplingType`,
`sample_from_indices`, `sample_pc`, `sample_pc_grouped` - plus the two PyTorch3D names it uses, over `ops.farthest_point_sample`
(csrc/am_fps.hip).  `install_into(module)` gives a module exactly the names the guarded import left missing.

What is and is not pinned:
  * the FPS itself is the exact greedy algorithm of include/actionmesh_amd.h (lowest index on ties), bit for bit against a numpy
    restatement; that PyTorch3D's CUDA kernel breaks ties identically is NOT pinned (PyTorch3D cannot be installed here);
  * `random_start_point=True` draws ONE `torch.randint(N, (B,))` from torch's global (CPU) generator per call; how PyTorch3D
    draws its start points is NOT pinned, so under the same seeds the two may start elsewhere;
  * every other draw (`torch.randperm` for RANDOM and for the `fps_max_points` pre-sampling) is made as the reference makes
    it, in the same order, so under one `torch.manual_seed` those indices are the reference's.
There is no CPU path: a CPU tensor that reaches the FPS raises (the reference's CPU branch is `fpsample`, another algorithm).
"""
from __future__ import annotations

from enum import Enum
from typing import Optional

import torch


class SamplingType(str, Enum):
    """Supported point cloud sampling strategies."""

    RANDOM = "random"
    FPS = "fps"
    FPS_FULL = "fps_full"


# ---- the two PyTorch3D names -----------------------------------------------------------------------------------------------------
def masked_gather(points: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """pytorch3d.ops.utils.masked_gather: points (B, P, D) gathered by idx (B, K) -> (B, K, D), or by idx (B, M, K) -> (B, M, K, D);
    an index of -1 is padding and yields zeros."""
    if len(idx) != len(points):
        raise ValueError("points and idx must have the same batch dimension")
    D = points.shape[-1]
    pad = idx.eq(-1)
    safe = idx.clone()
    safe[pad] = 0
    if idx.ndim == 3:
        src = points[:, :, None, :].expand(-1, -1, idx.shape[2], -1)
        out = src.gather(1, safe[..., None].expand(-1, -1, -1, D))
    elif idx.ndim == 2:
        out = points.gather(1, safe[..., None].expand(-1, -1, D))
    else:
        raise ValueError(f"idx format is not supported {tuple(idx.shape)}")
    out[pad] = 0.0
    return out


def _fps_core(points: torch.Tensor, n_samples: int, start_idx: Optional[torch.Tensor]) -> torch.Tensor:
    """(B, N, D) -> int64 (B, n_samples): the HIP kernel, every channel of `points` in the distance.  The one place the FPS
    arithmetic enters this module (tests/test_fps_cpu.py substitutes its numpy restatement here to compare the orchestration
    with the reference's on the CPU)."""
    from . import ops
    return ops.farthest_point_sample(points, n_samples, start_idx=start_idx).long()


def _random_start(points: torch.Tensor) -> torch.Tensor:
    return torch.randint(points.shape[1], (points.shape[0],))


def sample_farthest_points(points: torch.Tensor, lengths: Optional[torch.Tensor] = None, K: int = 50,
                           random_start_point: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """pytorch3d.ops.sample_farthest_points for equal-length clouds: (B, N, D) -> (points (B, K, D), indices int64 (B, K)).
    `lengths` (ragged batches) and K > N (padding with -1) are not supported: the reference uses neither."""
    if lengths is not None:
        raise NotImplementedError("sample_farthest_points: `lengths` (ragged batches) is not supported")
    if points.ndim != 3:
        raise ValueError(f"Expected 3-D tensor (B, N, D), got {points.ndim}-D")
    if not 1 <= K <= points.shape[1]:
        raise NotImplementedError(f"sample_farthest_points: K ({K}) must be within 1 .. N ({points.shape[1]})")
    start = _random_start(points) if random_start_point else None
    indices = _fps_core(points, K, start)
    return masked_gather(points, indices), indices


# ---- low-level helpers -----------------------------------------------------------------------------------------------------------
def _distance_input(points: torch.Tensor, sampling_type: SamplingType) -> torch.Tensor:
    return points[..., :3] if sampling_type == SamplingType.FPS else points


def _farthest_point_sample(
    points: torch.Tensor,
    n_samples: int,
    random_start_point: bool = True,
    sampling_type: SamplingType = SamplingType.FPS,
) -> tuple[torch.Tensor, torch.Tensor]:
    """FPS on a (B, N, D) cloud: FPS measures distances on XYZ only, FPS_FULL on all D channels; all D are gathered."""
    if points.ndim != 3:
        raise ValueError(f"Expected 3-D tensor (B, N, D), got {points.ndim}-D")
    _, indices = sample_farthest_points(_distance_input(points, sampling_type), K=n_samples, random_start_point=random_start_point)
    return masked_gather(points, indices), indices


def sample_from_indices(
    points: torch.Tensor,
    indices: torch.Tensor,
) -> torch.Tensor:
    """Gather points (B, N_PTS, D) by indices (B, M) or (1, M) -> (B, M, D)."""
    if points.ndim != 3:
        raise ValueError(f"Expected 3-D points, got {points.ndim}-D")
    if indices.ndim != 2:
        raise ValueError(f"Expected 2-D indices, got {indices.ndim}-D")
    if indices.shape[0] == 1:
        indices = indices.expand(points.shape[0], -1)
    if indices.shape[0] != points.shape[0]:
        raise ValueError(f"Batch size mismatch: points {points.shape[0]} vs indices {indices.shape[0]}")
    return masked_gather(points, indices)


def _sample_identity(points: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    return points, torch.arange(points.shape[1], device=points.device).reshape(1, -1)


def _randperm_indices(points: torch.Tensor, n_keep: int) -> torch.Tensor:
    """One torch.randperm per batch element, in batch order, on the global generator (the reference's order of draws)."""
    n_pts = points.shape[1]
    return torch.stack([torch.randperm(n_pts)[:n_keep] for _ in range(points.shape[0])]).to(points.device)


def _sample_random(points: torch.Tensor, n_samples: int) -> tuple[torch.Tensor, torch.Tensor]:
    indices = _randperm_indices(points, n_samples)
    return sample_from_indices(points, indices), indices


def _fold_chunks(dist_in: torch.Tensor, fps_chunks: int) -> Optional[torch.Tensor]:
    """(B, C * n, D) -> the view (B * C, n, D) whose entry b * C + c is chunk c of cloud b, when the chunks are equal and the strides
    allow it without a copy; None otherwise (the caller then runs chunk by chunk)."""
    B, n_pre, D = dist_in.shape
    if fps_chunks <= 1 or n_pre % fps_chunks != 0:
        return None
    try:
        return dist_in.view(B * fps_chunks, n_pre // fps_chunks, D)
    except RuntimeError:
        return None


def _sample_fps(
    points: torch.Tensor,
    n_samples: int,
    sampling_type: SamplingType,
    fps_max_points: Optional[int],
    fps_random: bool,
    fps_chunks: int,
) -> tuple[torch.Tensor, torch.Tensor]:
    """FPS with the optional random pre-sampling to at most `fps_max_points` (never fewer than n_samples) and the split into
    `fps_chunks` chunks along the point axis, each sampled on its own.  As in the reference, the indices returned address the
    PRE-SAMPLED cloud, chunk k's offset by k * (n_pre // fps_chunks)."""
    if fps_max_points is not None:
        n_pre = max(fps_max_points, n_samples)
        points_pre = sample_from_indices(points, _randperm_indices(points, n_pre))
    else:
        n_pre = points.shape[1]
        points_pre = points
    if n_pre <= n_samples:
        return points_pre, torch.arange(points_pre.shape[1], device=points.device).reshape(1, -1)

    chunk_size = n_samples // fps_chunks
    batch_size = points_pre.shape[0]
    folded = _fold_chunks(_distance_input(points_pre, sampling_type), fps_chunks)
    if folded is not None:
        # equal chunks: one launch, the chunks as extra batch entries; the start points are drawn chunk by chunk as the loop would
        start = None
        if fps_random:
            start = torch.stack([_random_start(folded[:batch_size]) for _ in range(fps_chunks)], dim=1).reshape(-1)
        indices = _fps_core(folded, chunk_size, start).view(batch_size, fps_chunks, chunk_size)
        offsets = torch.arange(fps_chunks, device=indices.device) * (n_pre // fps_chunks)
        indices = (indices + offsets[None, :, None]).reshape(batch_size, fps_chunks * chunk_size)
        return masked_gather(points_pre, indices), indices

    points_list: list[torch.Tensor] = []
    indices_list: list[torch.Tensor] = []
    for chunk_id, chunk in enumerate(points_pre.chunk(fps_chunks, dim=1)):
        chunk_out, chunk_indices = _farthest_point_sample(chunk, n_samples=chunk_size, random_start_point=fps_random,
                                                          sampling_type=sampling_type)
        points_list.append(chunk_out)
        indices_list.append(chunk_indices + chunk_id * (n_pre // fps_chunks))
    return torch.cat(points_list, dim=1), torch.cat(indices_list, dim=1)


# ---- the reference's entry points ------------------------------------------------------------------------------------------------
def sample_pc(
    points: torch.Tensor,
    n_samples: int,
    sampling_type: SamplingType | str = SamplingType.RANDOM,
    fps_max_points: Optional[int] = None,
    fps_random: bool = True,
    fps_chunks: int = 1,
) -> tuple[torch.Tensor, torch.Tensor]:
    """Sample `n_samples` points from a batched cloud (B, N_PTS, D): RANDOM, FPS (distances on XYZ) or FPS_FULL (on all D).
    Returns (sampled points (B, n_samples, D), int64 indices (B, n_samples) or (1, n_samples)); a cloud with no more than
    n_samples points comes back unchanged."""
    if not isinstance(points, torch.Tensor):
        raise TypeError(f"Expected torch.Tensor, got {type(points)}")
    if points.ndim != 3:
        raise ValueError(f"Expected 3-D (B, N_PTS, D), got {points.ndim}-D")
    if n_samples % fps_chunks != 0:
        raise ValueError(f"n_samples ({n_samples}) must be divisible by fps_chunks ({fps_chunks})")
    if isinstance(sampling_type, str):
        sampling_type = SamplingType(sampling_type)
    if points.shape[1] <= n_samples:
        return _sample_identity(points)
    if sampling_type is SamplingType.RANDOM:
        return _sample_random(points, n_samples)
    if sampling_type.value.startswith("fps"):
        return _sample_fps(points, n_samples, sampling_type, fps_max_points, fps_random, fps_chunks)
    raise ValueError(f"Unsupported sampling type: {sampling_type}")


def sample_pc_grouped(
    points: torch.Tensor,
    n_samples: int,
    n_grouped_frames: int,
    sampling_type: SamplingType | str = SamplingType.FPS,
    fps_max_points: Optional[int] = None,
    fps_random: bool = True,
    fps_chunks: int = 1,
) -> tuple[torch.Tensor, torch.Tensor]:
    """points (B*T, N_PTS, D) with T = n_grouped_frames: sample on the first frame of every batch element and use its indices
    for all T frames.  Returns (sampled points (B*T, n_samples, D), indices (B*T, n_samples))."""
    if isinstance(sampling_type, str):
        sampling_type = SamplingType(sampling_type)
    first = points.reshape(-1, n_grouped_frames, *points.shape[1:])[:, 0]
    _, indices = sample_pc(points=first, n_samples=n_samples, sampling_type=sampling_type, fps_max_points=fps_max_points,
                           fps_random=fps_random, fps_chunks=fps_chunks)
    indices = indices.unsqueeze(1).repeat(1, n_grouped_frames, 1).flatten(0, 1)
    return masked_gather(points, indices), indices


# ---- seam S7 ---------------------------------------------------------------------------------------------------------------------
SEAM_NAMES = ("sample_pc", "sample_pc_grouped", "masked_gather", "_is_pytorch3d_available")
_MISSING = object()


def install_into(module) -> dict:
    """Give `module` - meant for `actionmesh.external.triposg` - the names its guarded import leaves missing without PyTorch3D
    (triposg.py:17-23): `sample_pc`, `sample_pc_grouped`, `masked_gather`, and `_is_pytorch3d_available = True`, the flag
    `TripoSGVAE.__init__` tests.  No `pytorch3d` module is registered anywhere: code that decides by `import pytorch3d` (the
    preview renderer) keeps deciding as before.  Returns what the names held, for `uninstall_from`."""
    saved = {name: getattr(module, name, _MISSING) for name in SEAM_NAMES}
    module.sample_pc = sample_pc
    module.sample_pc_grouped = sample_pc_grouped
    module.masked_gather = masked_gather
    module._is_pytorch3d_available = True
    return saved


def uninstall_from(module, saved: dict) -> None:
    for name, value in saved.items():
        if value is _MISSING:
            if hasattr(module, name):
                delattr(module, name)
        else:
            setattr(module, name, value)
