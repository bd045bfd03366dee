"""ActionBench Chamfer metrics on the device (the end-to-end quality gate of the hot path).

Mirrors of the reference's actionbench/chamfer.py with the same names, arguments and sampling (numpy RandomState
permutations with the reference's seeds); the nearest-neighbour searches - scipy KD-trees over 100 000-point clouds in
the reference - run as one exact brute-force kernel (am_nn_search, fp64 arithmetic in the KD-tree's summation order), so
indices and distances are the reference's bit for bit; the final sqrt / mean reductions stay on the host in numpy exactly
as the reference has them.  No CPU fallback: inputs are moved to `device` (default cuda:0) and the library must be loaded.

Every search takes `nn`: "brute" (am_nn_search, the default of the library functions) or "grid" (am_nn_grid_*: the same indices and
distances bit for bit through a uniform grid, so every metric and the ICP's whole trajectory are the same numbers).
The ICP takes `step` / `icp`: "autograd" (the default: the graph over the two searches) or "fused" (am_icp_step: one device step per
iteration and no host read inside the loop; deterministic, not the autograd trajectory's bits).

The second half is the reference's dataset evaluator (actionbench/evaluate_dataset.py) with its names, defaults and file formats -
uid/surfaces.npy against uid/mesh_*.glb, a CSV and a summary JSON, resumable - on the stdlib's csv / json instead of pandas, a natural
sort key instead of natsort, and mesh_io.load_glb instead of trimesh:  python -m actionmesh_amd.actionbench --gt_root ... --pred_root ...
"""
from __future__ import annotations

import argparse
import csv
import dataclasses
import json
import logging
import math
import re
from dataclasses import dataclass, field
from pathlib import Path
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import mesh_io, ops

logger = logging.getLogger(__name__)

NN_METHODS = ("brute", "grid")
# The evaluator's default method: whichever profiles/nn_grid.json (tools/nn_grid_timing.py) measured faster on a whole gradient_icp by
# more than the spread between repeats, else "brute" (DESIGN section 6, row N12).
EVALUATOR_NN = "brute"
ICP_STEPS = ("autograd", "fused")
# The evaluator's ICP iteration: "autograd" (the graph below, the default) or "fused" (am_icp_step: matching, gradient, Adam step and
# best-so-far record on the device, no host read inside the loop; profiles/icp_fused.json).
EVALUATOR_ICP = "autograd"


def _search(points: torch.Tensor, queries: torch.Tensor, precise: bool, nn: str, check: bool = True):
    if nn not in NN_METHODS:
        raise ValueError(f"nn must be one of {NN_METHODS}, got {nn!r}")
    fn = ops.nearest_neighbors if nn == "brute" else ops.nearest_neighbors_grid
    return fn(points, queries, precise=precise, check=check)


def _dev(t, device) -> torch.Tensor:
    t = torch.as_tensor(t)
    device = torch.device(device) if device is not None else (t.device if t.is_cuda else torch.device("cuda:0"))
    return t.to(device=device, dtype=torch.float32).contiguous()


def nearest(points, queries, device=None, nn: str = "brute") -> Tuple[np.ndarray, np.ndarray]:
    """KDTree(points).query(queries) of chamfer.py: (distances float64, indices int64) as numpy arrays."""
    p, q = _dev(points, device), _dev(queries, device)
    idx, d2 = _search(p, q.to(p.device), True, nn)
    return np.sqrt(d2.cpu().numpy()), idx.cpu().numpy().astype(np.int64)


def compute_chamfer_score(pred, gt, n: int = 10_000, seed: int = 44, device=None, nn: str = "brute") -> float:
    """Symmetric Chamfer distance between two point clouds (actionbench/chamfer.py:13-52).  pred (N, 3), gt (M, 3);
    at most `n` query points per direction, drawn with the reference's RandomState(seed) / RandomState(seed + 1)."""
    pred_t, gt_t = torch.as_tensor(pred), torch.as_tensor(gt)
    rng_pred = np.random.RandomState(seed=seed)
    rng_gt = np.random.RandomState(seed=seed + 1)
    indices_pred = rng_pred.permutation(len(pred_t))[:n] if 0 < n < len(pred_t) else np.arange(len(pred_t))
    indices_gt = rng_gt.permutation(len(gt_t))[:n] if 0 < n < len(gt_t) else np.arange(len(gt_t))
    p, g = _dev(pred_t, device), _dev(gt_t, device)
    g = g.to(p.device)
    d1, _ = nearest(p, g[torch.from_numpy(indices_gt).to(p.device)], nn=nn)
    d2, _ = nearest(g, p[torch.from_numpy(indices_pred).to(p.device)], nn=nn)
    return float(np.mean(d1) + np.mean(d2))


def compute_motion_chamfer_score(preds, gts, device=None, nn: str = "brute") -> float:
    """Motion Chamfer distance over a sequence (actionbench/chamfer.py:55-86): correspondences from the first frame,
    distances over all frames.  preds (T, P, 3), gts (T, Q, 3)."""
    preds_t, gts_t = torch.as_tensor(preds), torch.as_tensor(gts)
    assert preds_t.shape[0] == gts_t.shape[0], "Mismatching number of timesteps"
    p, g = _dev(preds_t, device), _dev(gts_t, device)
    g = g.to(p.device)
    idx_gt_to_pred, _ = _search(p[0].contiguous(), g[0].contiguous(), True, nn)
    idx_pred_to_gt, _ = _search(g[0].contiguous(), p[0].contiguous(), True, nn)
    # the gathers and the fp32 differences on the device; norms and means in numpy like the reference (float32 data)
    diff1 = (p[:, idx_gt_to_pred.long(), :] - g).cpu().numpy()
    diff2 = (g[:, idx_pred_to_gt.long(), :] - p).cpu().numpy()
    d1 = np.linalg.norm(diff1, axis=-1).mean(axis=0)
    d2 = np.linalg.norm(diff2, axis=-1).mean(axis=0)
    return float(np.mean(d1) + np.mean(d2))


# ---------------------------------------------------------------------------------------------------------------- ICP
# actionbench/icp.py + benchmark.py.  The reference leans on pytorch3d (chamfer_distance, rotation_6d_to_matrix,
# euler_angles_to_matrix, Transform3d), which is not installable offline: the few formulas used are restated below from
# their published definitions (parity of this half is therefore UNPINNED - see oracle/actionbench_oracle.py - while the
# Chamfer metrics above are pinned to the reference's own code).  The 24 x 200 x 2 nearest-neighbour searches of
# gradient_icp run as batched am_nn_search launches (fp32, like pytorch3d's knn); the gradient flows through the matched
# pairs exactly as in pytorch3d's chamfer_distance (indices are constants of the backward pass).

def _axis_rotation(axis: str, angle: torch.Tensor) -> torch.Tensor:
    c, s, one, zero = torch.cos(angle), torch.sin(angle), torch.ones_like(angle), torch.zeros_like(angle)
    flat = {"X": (one, zero, zero, zero, c, -s, zero, s, c),
            "Y": (c, zero, s, zero, one, zero, -s, zero, c),
            "Z": (c, -s, zero, s, c, zero, zero, zero, one)}[axis]
    return torch.stack(flat, -1).reshape(angle.shape + (3, 3))


def euler_angles_to_matrix(euler_angles: torch.Tensor, convention: str = "XYZ") -> torch.Tensor:
    """pytorch3d.transforms.euler_angles_to_matrix: R = R_c0(a0) R_c1(a1) R_c2(a2)."""
    m = [_axis_rotation(c, a) for c, a in zip(convention, torch.unbind(euler_angles, -1))]
    return m[0] @ m[1] @ m[2]


def rotation_6d_to_matrix(d6: torch.Tensor) -> torch.Tensor:
    """pytorch3d.transforms.rotation_6d_to_matrix (Zhou et al. 2019): Gram-Schmidt of the two 3-vectors, rows b1, b2, b1 x b2."""
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = torch.nn.functional.normalize(a1, dim=-1)
    b2 = torch.nn.functional.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=-1)), dim=-2)


def canonical_rotation_matrices() -> torch.Tensor:
    """icp.py:19-51: the 24 axis-aligned orientations."""
    d = torch.pi / 180
    azim = torch.tensor([0] * 4 + [90] * 4 + [180] * 4 + [270] * 4 + [0] * 4 + [90] * 4, dtype=torch.float32) * d
    elev = torch.tensor([0] * 16 + [90] * 2 + [-90] * 2 + [90] * 2 + [-90] * 2, dtype=torch.float32) * d
    roll = torch.tensor([0, 90, 180, 270] * 4 + [0, 90] * 4, dtype=torch.float32) * d
    return euler_angles_to_matrix(torch.stack((azim, elev, roll), dim=-1), convention="XYZ")


class ScaleRotateTranslate:
    """What icp.py:108-111 returns (Scale(s).compose(Rotate(R), Translate(T)), row-vector convention): p' = (s * p) @ R + T,
    one transform or a stack of K of them applied to K point clouds."""

    def __init__(self, R: torch.Tensor, T: torch.Tensor, s: torch.Tensor):
        self.R, self.T, self.s = R.reshape(-1, 3, 3), T.reshape(-1, 3), s.reshape(-1, 3)

    def __len__(self) -> int:
        return self.R.shape[0]

    def stack(self, *others: "ScaleRotateTranslate") -> "ScaleRotateTranslate":
        items = (self,) + others
        return ScaleRotateTranslate(torch.cat([t.R for t in items]), torch.cat([t.T for t in items]), torch.cat([t.s for t in items]))

    def transform_points(self, points: torch.Tensor) -> torch.Tensor:
        p = points if points.dim() == 3 else points[None]
        out = (self.s[:, None, :] * p) @ self.R + self.T[:, None, :]
        return out if points.dim() == 3 else out[0]


class _GatherRows(torch.autograd.Function):
    """src (B, N, 3), index (B, M) -> src[b, index[b, m]] (B, M, 3), like torch.gather on the expanded index.  The backward sums the rows
    that share a source point in a FIXED order (index_put_ with accumulate: sorted keys, no float atomics), so two runs with the same
    matches - or a brute-force and a grid run - follow the same optimiser trajectory bit for bit; torch.gather's scatter-add backward
    adds with float atomics in whatever order the waves arrive."""

    @staticmethod
    def forward(ctx, src, index):
        B, N, _ = src.shape
        flat = (index.long() + torch.arange(B, device=src.device)[:, None] * N).reshape(-1)
        ctx.save_for_backward(flat)
        ctx.shape = src.shape
        return src.reshape(B * N, -1)[flat].reshape(B, index.shape[1], -1)

    @staticmethod
    def backward(ctx, grad):
        (flat,) = ctx.saved_tensors
        B, N, C = ctx.shape
        out = torch.zeros((B * N, C), dtype=grad.dtype, device=grad.device)
        out.index_put_((flat,), grad.reshape(-1, C), accumulate=True)
        return out.reshape(B, N, C), None


def chamfer_distance_sq(x: torch.Tensor, y: torch.Tensor, nn: str = "brute", y_grid: Optional["ops.NnGrid"] = None) -> torch.Tensor:
    """pytorch3d.loss.chamfer_distance(x, y, batch_reduction=None)[0]: per batch entry, mean_i min_j |x_i - y_j|^2 +
    mean_j min_i |y_j - x_i|^2; differentiable w.r.t. both clouds through the matched pairs.
    nn="grid": both searches go through grids, and each cloud's own cell order is the order in which the lanes of the OTHER search
    pick it as queries.  `y_grid`: the grid of y built by the caller (gradient_icp: one grid of pc_gt for the whole optimisation,
    shared by the batch); the grid of x is built here."""
    if nn not in NN_METHODS:
        raise ValueError(f"nn must be one of {NN_METHODS}, got {nn!r}")
    with torch.no_grad():
        xd, yd = x.detach().contiguous(), y.detach().contiguous()
        if nn == "brute":
            ixy, _ = ops.nearest_neighbors(yd, xd, precise=False, check=False)
            iyx, _ = ops.nearest_neighbors(xd, yd, precise=False, check=False)
            ops.nn_indices_valid(ixy, iyx)    # one host read for both searches (the ICP loop reads its loss once per iteration anyway)
        else:
            gy = ops.nn_grid_build(yd) if y_grid is None else y_grid
            gx = ops.nn_grid_build(xd)
            ixy, _ = ops.nn_grid_search(gy, xd, precise=False, query_order=gx.order, check=False)
            iyx, _ = ops.nn_grid_search(gx, yd, precise=False, query_order=gy.order, check=False)
            ops.nn_grid_valid([gx, gy], ixy, iyx)
    gx = _GatherRows.apply(y, ixy)
    gy = _GatherRows.apply(x, iyx)
    return (x - gx).pow(2).sum(-1).mean(1) + (y - gy).pow(2).sum(-1).mean(1)


@torch.enable_grad()
def gradient_icp(pc_pred: torch.Tensor, pc_gt: torch.Tensor, lr: float = 0.01, n_iter: int = 200, _chamfer=None,
                 nn: str = "brute", step: str = "autograd") -> ScaleRotateTranslate:
    """icp.py:54-111: the similarity (anisotropic scale) transform from pc_pred (P, 3) to pc_gt (Q, 3): Adam on a 6-D rotation,
    a translation and a per-axis scale from 24 canonical starting orientations at once; the best loss seen wins.
    nn="grid": ONE grid over pc_gt for the call, shared by the 24 candidates; the grid over the 24 transformed clouds is rebuilt every
    iteration.  The matched indices are brute force's, so the optimiser's trajectory and the result are the same bits.
    step="fused": every iteration is one am_icp_step (ops.icp_step) - the same matching, the gradient from 13 sums over the matched
    pairs, Adam and the best-so-far record in fp64 on the device - and the host reads `best` and the flag once, after the loop.  Its
    trajectory is deterministic but not the autograd one's bits (fp64 sums against fp32 ones); brute-force matching only."""
    if nn not in NN_METHODS:
        raise ValueError(f"nn must be one of {NN_METHODS}, got {nn!r}")
    if step not in ICP_STEPS:
        raise ValueError(f"step must be one of {ICP_STEPS}, got {step!r}")
    if step == "fused":
        if nn != "brute" or _chamfer is not None:
            raise ValueError('step="fused" matches by brute force inside am_icp_step: it takes neither nn="grid" nor _chamfer')
        return _gradient_icp_fused(pc_pred, pc_gt, lr, n_iter)
    if _chamfer is not None:
        chamfer = _chamfer
    elif nn == "grid":
        gt_grid = ops.nn_grid_build(pc_gt.detach().float().contiguous())
        chamfer = lambda x, y: chamfer_distance_sq(x, y, nn="grid", y_grid=gt_grid)      # noqa: E731
    else:
        chamfer = chamfer_distance_sq
    device = pc_pred.device
    R_init = canonical_rotation_matrices().to(device)
    n_rots = len(R_init)
    pred = pc_pred.detach().float()[None].expand(n_rots, -1, -1)
    gt = pc_gt.detach().float()[None].expand(n_rots, -1, -1).contiguous()
    T = torch.nn.Parameter(torch.zeros(n_rots, 3, device=device))
    R_6d = torch.nn.Parameter(torch.tensor([[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]], device=device).repeat(n_rots, 1))
    s = torch.nn.Parameter(torch.ones(n_rots, 3, device=device))
    opt = torch.optim.Adam(params=[T, R_6d, s], lr=lr)
    best_loss, best = float("inf"), None
    for _ in range(n_iter):
        opt.zero_grad()
        R = R_init @ rotation_6d_to_matrix(R_6d)
        loss = chamfer(s[:, None] * pred @ R + T[:, None], gt)
        loss.mean().backward()
        opt.step()
        min_loss, idx = loss.detach().min(0)
        if min_loss.item() < best_loss:
            best_loss = min_loss.item()
            best = (R[idx:idx + 1].detach().clone(), T[idx:idx + 1].detach().clone(), s[idx:idx + 1].detach().clone())
    out = ScaleRotateTranslate(*best)
    out.loss = best_loss
    return out


def _gradient_icp_fused(pc_pred: torch.Tensor, pc_gt: torch.Tensor, lr: float, n_iter: int) -> ScaleRotateTranslate:
    pred, gt = pc_pred.detach().float().contiguous(), pc_gt.detach().float().contiguous()
    R_init = canonical_rotation_matrices().to(pred.device).contiguous()
    state = ops.IcpState(len(R_init), pred.device)
    for t in range(1, n_iter + 1):
        ops.icp_step(state, pred, gt, R_init, t, lr=lr)
    best, flag = state.best.cpu(), int(state.out_flag.cpu())      # the only host reads: both after the loop
    if flag & ops.L.ICP_NO_NEIGHBOUR:
        raise ValueError(ops.NO_NEIGHBOUR_TEXT)
    dev = pred.device
    out = ScaleRotateTranslate(best[:9].reshape(1, 3, 3).to(dev), best[9:12].reshape(1, 3).to(dev), best[12:15].reshape(1, 3).to(dev))
    out.loss = float(best[15])
    return out


def sample_point_cloud(point_cloud: torch.Tensor, n_pts: int, seed: int = 44) -> torch.Tensor:
    """actionbench/sample_point_cloud.py:12-36: one RandomState(seed) permutation shared by all timesteps."""
    n_src = point_cloud.shape[1]
    if n_src <= n_pts:
        return point_cloud
    idx = torch.from_numpy(np.random.RandomState(seed=seed).permutation(n_src)[:n_pts]).long()
    return point_cloud[:, idx.to(point_cloud.device)]


def compute_chamfer_3d_4d(gt_pc: torch.Tensor, pred_pc: torch.Tensor, device="cuda:0", is_4D: bool = False,
                          pred_pc_4D: Optional[torch.Tensor] = None, n_pts_icp: int = 10_000, seed: int = 44,
                          n_iter: int = 200, nn: str = "brute", icp: str = "autograd") -> Tuple[float, float, float]:
    """benchmark.py:67-153 from point clouds: gt_pc (T, N, 3), pred_pc (T, M, 3) sampled per frame, pred_pc_4D (T, M, 3)
    sampled with frame-to-frame correspondence (is_4D).  (The reference samples these from trimesh objects with trimesh /
    pytorch3d samplers - sample_mesh.py - whose random streams are theirs; hand it the same clouds and the rest follows
    benchmark.py line by line.)  Returns (cd_3d: per-frame ICP, cd_4d: first-frame ICP, cd_motion)."""
    icp_nn = "brute" if icp == "fused" else nn         # the fused iteration matches by brute force; `nn` still serves the metrics
    n_ts = pred_pc.shape[0]
    pred_pc_icp = sample_point_cloud(pred_pc, n_pts=n_pts_icp, seed=seed)
    gt_pc_icp = sample_point_cloud(gt_pc, n_pts=n_pts_icp, seed=seed)
    pred_pc, gt_pc = _dev(pred_pc, device), _dev(gt_pc, device)
    pred_pc_icp, gt_pc_icp = _dev(pred_pc_icp, device), _dev(gt_pc_icp, device)
    icp_list = [gradient_icp(pc_gt=gt_pc_icp[k], pc_pred=pred_pc_icp[k], lr=0.01, n_iter=n_iter, nn=icp_nn, step=icp) for k in range(n_ts)]
    icp_3d = icp_list[0].stack(*icp_list[1:])
    icp_u4d = gradient_icp(pc_gt=gt_pc_icp[0], pc_pred=pred_pc_icp[0], lr=0.01, n_iter=n_iter, nn=icp_nn, step=icp)
    aligned_3d, aligned_u4d = icp_3d.transform_points(pred_pc), icp_u4d.transform_points(pred_pc)
    cd_3d = np.mean([compute_chamfer_score(gt=gt_pc[k], pred=aligned_3d[k], nn=nn) for k in range(n_ts)])
    cd_4d = np.mean([compute_chamfer_score(gt=gt_pc[k], pred=aligned_u4d[k], nn=nn) for k in range(n_ts)])
    cd_motion = 0.0
    if is_4D:
        if pred_pc_4D is None:
            raise ValueError("is_4D needs pred_pc_4D (the synchronized sampling of the predicted meshes)")
        cd_motion = compute_motion_chamfer_score(preds=icp_u4d.transform_points(_dev(pred_pc_4D, device)), gts=gt_pc, nn=nn)
    return float(cd_3d), float(cd_4d), float(cd_motion)


def sample_meshes(vertices, faces, n_pts: int = 100_000, synchronized: bool = False, seed: int = 44) -> torch.Tensor:
    """actionbench/sample_mesh.py:216-243 on the Stage-II vertex stack: vertices (T, V, 3) sharing `faces` (F, 3) -> (T, n_pts, 3)
    surface samples, area-weighted faces and uniform barycentric coordinates (w0 = 1 - sqrt(u), w1 = sqrt(u)(1 - v), w2 = sqrt(u) v,
    sample_mesh.py:33-57).  `synchronized`: one draw of (face, barycentric) on frame 0 applied to every frame (point
    correspondence across the sequence, :169-190); otherwise an independent draw per frame with seed + frame (:237-243).
    The random STREAMS are torch's (seeded generator on the tensor's device), not trimesh's / pytorch3d's, so the clouds are
    statistically - not bitwise - the reference's."""
    v = torch.as_tensor(vertices, dtype=torch.float32)
    f = torch.as_tensor(faces).long().to(v.device)
    if v.dim() != 3 or v.shape[-1] != 3 or f.dim() != 2 or f.shape[-1] != 3 or f.numel() == 0:
        raise ValueError(f"sample_meshes: need (T, V, 3) vertices and (F >= 1, 3) faces, got {tuple(v.shape)} / {tuple(f.shape)}")
    if not torch.isfinite(v).all():
        raise ValueError("Meshes contain nan or inf.")

    def draw(frame: int, s: int):
        g = torch.Generator(device=v.device).manual_seed(s)
        tri = v[frame][f]                                                       # (F, 3, 3)
        areas = 0.5 * torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).norm(dim=-1)
        face = torch.multinomial(areas, n_pts, replacement=True, generator=g)
        uv = torch.rand((2, n_pts), device=v.device, generator=g)
        su = uv[0].sqrt()
        return face, torch.stack((1.0 - su, su * (1.0 - uv[1]), su * uv[1]), dim=-1)

    def apply(frame: int, face, w):
        tri = v[frame][f[face]]                                                 # (n, 3, 3)
        return (w[:, :, None] * tri).sum(dim=1)

    if synchronized:
        face, w = draw(0, seed)
        return torch.stack([apply(t, face, w) for t in range(v.shape[0])])
    return torch.stack([apply(t, *draw(t, seed + t)) for t in range(v.shape[0])])


# ------------------------------------------------------------------------------------------------------ dataset evaluator
# actionbench/evaluate_dataset.py.  Expected structure:  GT {gt_root}/{uid}/surfaces.npy (T, N, >= 3) point clouds, predictions
# {pred_root}/{uid}/mesh_*.glb.  Meshes are read with mesh_io.load_glb, which reads the triangle primitives of a binary glTF 2.0
# container and concatenates them; it does NOT read Draco-compressed geometry, interleaved buffer views, non-triangle primitives or
# any other file format, and applies no node transforms.  Such a file raises, and the sample gets status "error" with the message,
# exactly as the reference's try / except records a trimesh failure.

@dataclass
class SampleResult:
    """Result for a single sample evaluation (the CSV's columns, in this order)."""
    uid: str
    cd_3d: float = float("nan")
    cd_4d: float = float("nan")
    cd_motion: float = float("nan")
    n_frames: int = 0
    status: str = "pending"
    error_message: str = ""


CSV_COLUMNS = [f.name for f in dataclasses.fields(SampleResult)]


@dataclass
class DatasetResults:
    """Aggregated results for the entire dataset."""
    samples: List[SampleResult] = field(default_factory=list)

    def add(self, result: SampleResult) -> None:
        self.samples.append(result)

    def rows(self) -> List[Dict]:
        return [dataclasses.asdict(s) for s in self.samples]

    def summary(self) -> Dict[str, float]:
        """Mean metrics over successful samples (the reference's keys)."""
        ok = [s for s in self.samples if s.status == "success"]
        n_total, n_success = len(self.samples), len(ok)
        out = {"n_total": n_total, "n_success": n_success, "n_failed": n_total - n_success,
               "success_rate": n_success / n_total if n_total > 0 else 0.0}
        for key in ("cd_3d", "cd_4d", "cd_motion"):
            out[f"{key}_mean"] = float(np.mean([getattr(s, key) for s in ok])) if ok else float("nan")
        return out


def natural_key(path) -> List:
    """Sort key under which mesh_2 comes before mesh_10: the digit runs of the name compare as numbers."""
    return [(0, int(t), "") if t.isdigit() else (1, 0, t.lower()) for t in re.split(r"(\d+)", str(path)) if t != ""]


def find_uids(gt_root: Path, pred_root: Path, mesh_pattern: str = "mesh_*.glb") -> List[str]:
    """All UIDs that exist in both the GT and the prediction directories, sorted."""
    gt_root, pred_root = Path(gt_root), Path(pred_root)
    gt_uids = {p.parent.name for p in gt_root.glob("*/surfaces.npy")}
    pred_uids = {p.relative_to(pred_root).parts[0] for p in pred_root.glob(f"*/{mesh_pattern}")}
    common = gt_uids & pred_uids
    logger.info(f"Found {len(gt_uids)} GT, {len(pred_uids)} pred, {len(common)} common")
    if not gt_uids:
        raise FileNotFoundError(f"No GT samples found in {gt_root}. Expected */surfaces.npy files.")
    if not pred_uids:
        raise FileNotFoundError(f"No predictions found in {pred_root}. Expected */{mesh_pattern} files.")
    if not common:
        raise ValueError(f"No common UIDs between GT and predictions. GT UIDs: {len(gt_uids)}, Pred UIDs: {len(pred_uids)}.")
    if gt_uids - pred_uids:
        logger.warning(f"Missing predictions: {len(gt_uids - pred_uids)}")
    if pred_uids - gt_uids:
        logger.warning(f"Missing GT: {len(pred_uids - gt_uids)}")
    return sorted(common)


def load_gt_surfaces(gt_path: Path) -> torch.Tensor:
    """surfaces.npy -> (T, N, 3) float32 positions (further channels, normals, are dropped)."""
    return torch.from_numpy(np.load(gt_path))[..., :3].float()


def load_pred_meshes(pred_dir: Path, n_frames: Optional[int] = None, pattern: str = "mesh_*.glb") -> List[Tuple[np.ndarray, np.ndarray]]:
    """The predicted meshes of a directory in natural filename order, the first `n_frames` of them: [(vertices (V, 3) float32,
    faces (F, 3) int64), ...]."""
    mesh_files = sorted(Path(pred_dir).glob(pattern), key=natural_key)
    if not mesh_files:
        raise FileNotFoundError(f"No mesh files found in {pred_dir}")
    if n_frames is not None:
        if len(mesh_files) < n_frames:
            raise ValueError(f"Not enough meshes: found {len(mesh_files)}, need {n_frames}")
        mesh_files = mesh_files[:n_frames]
    return [mesh_io.load_glb(p) for p in mesh_files]


def _one_topology(meshes) -> bool:
    v0, f0 = meshes[0]
    return all(v.shape == v0.shape and f.shape == f0.shape and np.array_equal(f, f0) for v, f in meshes[1:])


def compute_chamfer_3d_4d_meshes(gt_pc: torch.Tensor, pred_meshes, device="cuda", is_4D: bool = False, n_pts_icp: int = 10_000,
                                 n_pts_chamfer: int = 100_000, seed: int = 44, n_iter: int = 200, nn: str = "brute",
                                 icp: str = "autograd") -> Tuple[float, float, float]:
    """benchmark.py:67-153 from meshes: sample (sample_meshes), then compute_chamfer_3d_4d.  Meshes of one topology are sampled as a
    vertex stack; per-frame topologies frame by frame (seed + frame, sample_mesh.py:237-243).  The synchronized sampling of is_4D
    needs one topology, as the reference's assertion does."""
    device = torch.device("cuda:0" if str(device) == "cuda" else device)
    one = _one_topology(pred_meshes)
    if is_4D and not one:
        raise AssertionError("synchronized sampling (is_4D) needs meshes of one topology")
    if one:
        verts = torch.from_numpy(np.stack([v for v, _ in pred_meshes])).to(device)
        faces = torch.from_numpy(pred_meshes[0][1]).to(device)
        pred_pc = sample_meshes(verts, faces, n_pts=n_pts_chamfer, synchronized=False, seed=seed)
        pred_pc_4d = sample_meshes(verts, faces, n_pts=n_pts_chamfer, synchronized=True, seed=seed) if is_4D else None
    else:
        pred_pc = torch.stack([sample_meshes(torch.from_numpy(v)[None].to(device), torch.from_numpy(f).to(device), n_pts=n_pts_chamfer,
                                             synchronized=False, seed=seed + t)[0] for t, (v, f) in enumerate(pred_meshes)])
        pred_pc_4d = None
    return compute_chamfer_3d_4d(gt_pc, pred_pc, device=device, is_4D=is_4D, pred_pc_4D=pred_pc_4d, n_pts_icp=n_pts_icp, seed=seed,
                                 n_iter=n_iter, nn=nn, icp=icp)


def evaluate_sample(uid: str, gt_root: Path, pred_root: Path, device: str = "cuda", n_pts_icp: int = 10_000, n_pts_chamfer: int = 100_000,
                    seed: int = 44, mesh_pattern: str = "mesh_*.glb", is_4d: bool = True, n_iter: int = 200, nn: str = EVALUATOR_NN,
                    _metrics: Optional[Callable] = None, icp: str = EVALUATOR_ICP) -> SampleResult:
    """Evaluate a single sample: SampleResult with the metrics, or with status "error" and the message.  `_metrics`: the function
    called as compute_chamfer_3d_4d_meshes is (tests inject one).  `icp` travels on only when it is not the default, so the default
    call is the one it was before the keyword existed."""
    icp_kw = {} if icp == EVALUATOR_ICP else {"icp": icp}
    metrics = compute_chamfer_3d_4d_meshes if _metrics is None else _metrics
    result = SampleResult(uid=uid)
    try:
        gt_path, pred_dir = Path(gt_root) / uid / "surfaces.npy", Path(pred_root) / uid
        if not gt_path.exists():
            result.status, result.error_message = "error", f"GT not found: {gt_path}"
            return result
        if not pred_dir.exists():
            result.status, result.error_message = "error", f"Pred dir not found: {pred_dir}"
            return result
        gt_pc = load_gt_surfaces(gt_path)
        result.n_frames = n_frames = gt_pc.shape[0]
        try:
            pred_meshes = load_pred_meshes(pred_dir, n_frames=n_frames, pattern=mesh_pattern)
        except (FileNotFoundError, ValueError) as e:
            result.status, result.error_message = "error", str(e)
            return result
        cd_3d, cd_4d, cd_motion = metrics(gt_pc=gt_pc, pred_meshes=pred_meshes, device=device, is_4D=is_4d, n_pts_icp=n_pts_icp,
                                          n_pts_chamfer=n_pts_chamfer, seed=seed, n_iter=n_iter, nn=nn, **icp_kw)
        result.cd_3d, result.cd_4d, result.cd_motion, result.status = float(cd_3d), float(cd_4d), float(cd_motion), "success"
    except Exception as e:           # the reference records every failure of a sample and goes on
        result.status, result.error_message = "error", str(e)
        logger.error(f"[{uid}] Error: {e}")
    return result


def _float(text: str) -> float:
    return float(text) if text not in ("", None) else float("nan")


def load_existing_results(output_csv: Path) -> Dict[str, SampleResult]:
    """uid -> SampleResult of an earlier run's CSV (empty when there is none)."""
    output_csv = Path(output_csv)
    if not output_csv.exists():
        return {}
    results = {}
    with open(output_csv, newline="") as f:
        for row in csv.DictReader(f):
            results[row["uid"]] = SampleResult(uid=row["uid"], cd_3d=_float(row["cd_3d"]), cd_4d=_float(row["cd_4d"]),
                                               cd_motion=_float(row["cd_motion"]), n_frames=int(float(row["n_frames"] or 0)),
                                               status=row["status"], error_message=row.get("error_message") or "")
    return results


def save_results(results: DatasetResults, output_path: Path) -> None:
    """The CSV (columns in SampleResult's order; a NaN is an empty cell, as pandas writes it) and <name>.summary.json beside it."""
    output_path = Path(output_path)
    output_path.parent.mkdir(parents=True, exist_ok=True)
    with open(output_path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=CSV_COLUMNS)
        w.writeheader()
        for row in results.rows():
            w.writerow({k: ("" if isinstance(v, float) and math.isnan(v) else repr(v) if isinstance(v, float) else v) for k, v in row.items()})
    with open(output_path.with_suffix(".summary.json"), "w") as f:
        json.dump(results.summary(), f, indent=2)


def evaluate_dataset(gt_root: str, pred_root: str, output_csv: Optional[str] = None, device: str = "cuda", n_pts_icp: int = 10_000,
                     n_pts_chamfer: int = 100_000, seed: int = 44, mesh_pattern: str = "mesh_*.glb", recompute: bool = False,
                     is_4d: bool = True, n_iter: int = 200, nn: str = EVALUATOR_NN, _metrics: Optional[Callable] = None,
                     icp: str = EVALUATOR_ICP) -> DatasetResults:
    """Evaluate all samples of the dataset.  Results are saved after each sample, and the successful rows of an existing CSV are
    taken over on restart (failed ones are retried) unless recompute=True."""
    if icp not in ICP_STEPS:
        raise ValueError(f"icp must be one of {ICP_STEPS}, got {icp!r}")
    icp_kw = {} if icp == EVALUATOR_ICP else {"icp": icp}
    gt_root, pred_root = Path(gt_root), Path(pred_root)
    output_path = Path(output_csv) if output_csv else None
    uids = find_uids(gt_root, pred_root, mesh_pattern)
    existing: Dict[str, SampleResult] = {}
    if output_path and not recompute:
        existing = load_existing_results(output_path)
        if existing:
            n_done = sum(1 for r in existing.values() if r.status == "success")
            logger.info(f"Loaded {len(existing)} existing results ({n_done} successful). Use --recompute to redo all.")
    results = DatasetResults()
    for uid in uids:
        if uid in existing and not recompute:
            prev = existing[uid]
            if prev.status == "success":
                results.add(prev)
                continue
            logger.info(f"[{uid}] Retrying previously failed sample")
        result = evaluate_sample(uid=uid, gt_root=gt_root, pred_root=pred_root, device=device, n_pts_icp=n_pts_icp, n_pts_chamfer=n_pts_chamfer,
                                 seed=seed, mesh_pattern=mesh_pattern, is_4d=is_4d, n_iter=n_iter, nn=nn, _metrics=_metrics, **icp_kw)
        results.add(result)
        if result.status == "success":
            logger.info(f"[{uid}] CD_3D={result.cd_3d:.3f}, CD_4D={result.cd_4d:.3f}, CD_Motion={result.cd_motion:.3f}")
        if output_path:
            save_results(results, output_path)
    if output_path:
        save_results(results, output_path)
        logger.info(f"Results saved to: {output_path}")
        logger.info(f"Summary saved to: {output_path.with_suffix('.summary.json')}")
    return results


def print_summary(results: DatasetResults) -> None:
    """Print a formatted summary of the evaluation results."""
    summary = results.summary()
    print("\n" + "=" * 60)
    print("EVALUATION SUMMARY")
    print("=" * 60)
    print("\nSamples:")
    print(f"  Total:   {summary['n_total']}")
    print(f"  Success: {summary['n_success']}")
    print(f"  Failed:  {summary['n_failed']}")
    print(f"  Rate:    {summary['success_rate']:.1%}")
    if summary["n_success"] > 0:
        print("\nMetrics (mean):")
        print(f"  CD_3D:     {summary['cd_3d_mean']:.3f}")
        print(f"  CD_4D:     {summary['cd_4d_mean']:.3f}")
        print(f"  CD_Motion: {summary['cd_motion_mean']:.3f}")
    failed = [s for s in results.samples if s.status != "success"]
    if failed:
        print(f"\nFailed samples ({len(failed)}):")
        for s in failed:
            print(f"  [{s.uid}] {s.status}: {s.error_message}")
    print("=" * 60 + "\n")


def main(argv=None) -> DatasetResults:
    parser = argparse.ArgumentParser(prog="python -m actionmesh_amd.actionbench",
                                     description="Evaluate 3D/4D reconstruction metrics across a dataset")
    parser.add_argument("--gt_root", type=str, required=True, help="Root directory containing GT surfaces (uid/surfaces.npy)")
    parser.add_argument("--pred_root", type=str, required=True, help="Root directory containing predictions (uid/mesh_*.glb)")
    parser.add_argument("--output_csv", type=str, default=None, help="Path to save results CSV")
    parser.add_argument("--device", type=str, default="cuda", help="Device for computation (a GPU: there is no CPU path)")
    parser.add_argument("--n_pts_icp", type=int, default=10_000, help="Number of points for ICP alignment")
    parser.add_argument("--n_pts_chamfer", type=int, default=100_000, help="Number of points for Chamfer computation")
    parser.add_argument("--seed", type=int, default=44, help="Random seed for reproducibility")
    parser.add_argument("--mesh_pattern", type=str, default="mesh_*.glb", help="Glob pattern for mesh files (default: mesh_*.glb)")
    parser.add_argument("--recompute", action="store_true", help="Recompute all samples even if already done")
    parser.add_argument("--3d-only", action="store_true", dest="three_d_only", help="Compute 3D metrics only (skip 4D/motion metrics)")
    parser.add_argument("--nn", choices=NN_METHODS, default=EVALUATOR_NN, help="Nearest-neighbour search: brute force or the grid (same numbers)")
    parser.add_argument("--icp", choices=ICP_STEPS, default=EVALUATOR_ICP,
                        help="ICP iteration: the autograd graph, or the fused device step (no host read inside the loop)")
    parser.add_argument("--n_iter", type=int, default=200, help="ICP iterations")
    args = parser.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(levelname)s - %(message)s")
    results = evaluate_dataset(gt_root=args.gt_root, pred_root=args.pred_root, output_csv=args.output_csv, device=args.device,
                               n_pts_icp=args.n_pts_icp, n_pts_chamfer=args.n_pts_chamfer, seed=args.seed, mesh_pattern=args.mesh_pattern,
                               recompute=args.recompute, is_4d=not args.three_d_only, n_iter=args.n_iter, nn=args.nn,
                               **({} if args.icp == EVALUATOR_ICP else {"icp": args.icp}))
    print_summary(results)
    return results


if __name__ == "__main__":
    main()
