"""Anchor-mesh preparation on tensors: the reference's `actionmesh/preprocessing/mesh_processor.py` - `merge_and_clean_mesh`,
`get_mesh_features`, `normalize_mesh` / `denormalize_mesh`, `normalize_mesh_to_bounds`, `sample_surface`,
`MeshPostprocessor.process_mesh` - with the same names and argument order, on the `(vertices, faces)` tensors the Stage-II path here
works on instead of a `trimesh.Trimesh`.  Everything stays on the input's device: the geometry (vertex normals, face areas, surface
samples) is HIP (`ops.vertex_normals`, `ops.face_areas`, `ops.surface_sample`, csrc/am_mesh.hip, contract in
include/actionmesh_amd.h); the vertex merge, the face filters and the re-indexing are integer keys - `torch.unique` / `sort` /
`scatter_reduce` on the same device, which also run on CPU tensors.  `process_mesh(..., decimation="hip")` decimates through
`mesh_decimate.decimate_mesh` (csrc/am_decimate.hip) between the clean-up and the floater removal; without the keyword it does not.

What is PINNED: the contract written in the header and in the docstrings here, against numpy fp64 restatements (tests/test_mesh_prep_*).
trimesh is not installable where this was written, so these are a recollection of its behaviour and UNPINNED:
  * `tol.merge` = 1e-8: vertices merge when `round(v * 1e8)` agrees in all three coordinates (MERGE_DIGITS);
  * `tol.zero` = 1e-13: the norm at or below which a face normal or a summed vertex normal is zero (AM_MESH_ZERO in the header);
  * the degeneracy rule of `nondegenerate_faces`: a repeated index, or a height over the longest edge below 1e-8 (DEGENERATE_HEIGHT);
  * the order of the merged vertices (here: by the lowest original index of each group, which also supplies the position);
  * the sampling recipe of `trimesh.sample.sample_surface`: `random(n)` for the faces, then `random((n, 2, 1))` for the barycentric
    pair, the fold `r -= 1; r = |r|` when `r0 + r1 > 1`, and the order in which origin and edge vectors are summed;
  * that a mesh which carries UVs or vertex normals merges on positions only (trimesh also compares those attributes; the tensors
    here have none).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import mesh_cleanup, ops
from .mesh_topology import MeshTopology, check_faces, check_mesh, referenced_vertices

MERGE_DIGITS = 8                # trimesh's tol.merge = 1e-8 as decimal digits
DEGENERATE_HEIGHT = 1e-8        # trimesh's nondegenerate_faces(height=tol.merge)

NO_IMAGE_MESSAGE = ("Some pre-merge vertices have no close match in the merged mesh ({count} of {total}). "
                    "merge_vertices() may have altered positions.")


def get_mesh_features(vertices: torch.Tensor, faces: torch.Tensor, with_normals: bool, topology: Optional[MeshTopology] = None) -> torch.Tensor:
    """Vertex positions, optionally with the normalised angle-weighted vertex normals: (V, 3|6) fp32 for (V, 3) vertices, (T, V, 3|6)
    for a stack of frames that share `faces`."""
    if not with_normals:
        return vertices.float()
    if topology is None:
        topology = MeshTopology(faces, vertices.shape[-2])
    return ops.vertex_normals(vertices, topology.faces, topology=topology, features=True)


class VertexFeatures:
    """`vertices (V, 3) -> (V, 6)` for a fixed face array: the `vertex_features` argument of `generate_vertex_animation`.  The
    topology is built on first use and kept."""

    def __init__(self, faces: torch.Tensor):
        check_faces(faces, "VertexFeatures")
        self.faces = faces
        self.topology: Optional[MeshTopology] = None

    def __call__(self, vertices: torch.Tensor) -> torch.Tensor:
        V = vertices.shape[-2]
        if self.topology is None or self.topology.n_vertices != V or self.topology.faces.device != vertices.device:
            self.topology = MeshTopology(self.faces.to(vertices.device), V)
        return get_mesh_features(vertices, self.topology.faces, True, topology=self.topology)


# ---- clean-up -------------------------------------------------------------------------------------------------------------------------
def _first_index(inverse: torch.Tensor, n_groups: int) -> torch.Tensor:
    """The lowest position of every group of `inverse` (int64 (n_groups,))."""
    pos = torch.arange(inverse.numel(), device=inverse.device)
    first = torch.full((n_groups,), inverse.numel(), dtype=torch.int64, device=inverse.device)
    return first.scatter_reduce(0, inverse, pos, reduce="amin")


def _clean(vertices: torch.Tensor, faces: torch.Tensor):
    """The four clean-up steps.  Returns (vertices', faces', map (V_original,) int64 with -1 where the vertex has no image, kept face
    indices)."""
    dev = vertices.device
    f = faces.long()
    if f.numel() and bool(((f < 0) | (f >= vertices.shape[0])).any()):          # one read: the gathers below index with these
        raise ValueError(f"mesh clean-up: a face names a vertex outside [0, {vertices.shape[0]})")
    # 1. merge
    key = torch.round(vertices.double() * float(10 ** MERGE_DIGITS)).to(torch.int64)
    groups, inverse = torch.unique(key, dim=0, return_inverse=True)
    n_groups = groups.shape[0]
    first = _first_index(inverse, n_groups)
    first_sorted, order = torch.sort(first)                         # merged vertices by their lowest member
    rank = torch.empty_like(order)
    rank[order] = torch.arange(n_groups, device=dev)
    merged_of = rank[inverse]                                       # original vertex -> merged vertex
    merged = vertices[first_sorted]
    f = merged_of[f]
    # 2. degenerate faces: a repeated index, or the fp64 height over the longest edge below DEGENERATE_HEIGHT.  Every product and
    # difference is its own torch call, so CPU and device round alike.
    p = merged.double()
    v0, v1, v2 = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    e1, e2, e3 = v1 - v0, v2 - v0, v2 - v1
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    norm = lambda x, y, z: torch.sqrt((x * x + y * y) + z * z)
    longest = torch.maximum(torch.maximum(norm(*e1.unbind(1)), norm(*e2.unbind(1))), norm(*e3.unbind(1)))
    repeated = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])
    keep = ~repeated & (norm(cx, cy, cz) / longest >= DEGENERATE_HEIGHT)          # 0 / 0 is NaN: dropped
    # 3. duplicate faces: the same vertex set whatever the winding; the first occurrence stays
    face_index = torch.nonzero(keep).reshape(-1)
    f = f[face_index]
    if f.shape[0]:
        sets, finv = torch.unique(torch.sort(f, dim=1).values, dim=0, return_inverse=True)
        is_first = _first_index(finv, sets.shape[0])[finv] == torch.arange(f.shape[0], device=dev)
        face_index, f = face_index[is_first], f[is_first]
    # 4. unreferenced vertices
    used, rank = referenced_vertices(f, n_groups)
    remap = torch.where(used, rank, torch.full_like(rank, -1))
    return merged[used], remap[f].to(faces.dtype), remap[merged_of], face_index


def merge_and_clean_mesh(vertices: torch.Tensor, faces: torch.Tensor, return_index: bool = False):
    """Merge duplicate vertices (GLB loading duplicates them at UV seams and hard edges) and clean the topology.  Steps, in order:
      1. vertices whose round(v * 1e8) (fp64 -> int64) agree in all three coordinates merge; the merged vertex keeps the position of
         its lowest-index member, and merged vertices are ordered by that lowest index;
      2. a face is dropped as degenerate when two of its indices are equal after the merge, or when its fp64 height over its longest
         edge, |e1 x e2| / longest edge, is below 1e-8;
      3. a face whose vertex set equals that of an earlier face is dropped, whatever the winding;
      4. vertices no remaining face references are dropped; the others keep their order.
    Returns (vertices', faces', vertex_merge_map (V_original,) int64, pre_merge_faces) - `vertices'[vertex_merge_map]` are the original
    vertices to the merge tolerance and `pre_merge_faces` is the input face array - and with `return_index` also the int64 indices
    of the kept faces.  The map comes straight from the merge and the re-index (the reference recovers it with a cKDTree because
    trimesh hides it).  An original vertex without a surviving image - one that no kept face reaches - raises AssertionError, as the
    reference's distance assertion does (one device-to-host read for that check)."""
    check_mesh(vertices, faces, "merge_and_clean_mesh")
    new_vertices, new_faces, merge_map, face_index = _clean(vertices, faces)
    missing = int((merge_map < 0).sum())
    if missing:
        raise AssertionError(NO_IMAGE_MESSAGE.format(count=missing, total=vertices.shape[0]))
    if return_index:
        return new_vertices, new_faces, merge_map, faces, face_index
    return new_vertices, new_faces, merge_map, faces


def process_mesh(vertices: torch.Tensor, faces: torch.Tensor, face_decimation: int = -1, floaters_threshold: float = 0.0,
                 decimation: Optional[str] = None, decimate_borders: str = "fixed"):
    """`MeshPostprocessor.process_mesh` on tensors, in the reference's order: the four clean-up steps of `merge_and_clean_mesh`, the
    quadric decimation to `face_decimation` faces, then - as the reference, only with floaters_threshold > 0 -
    `mesh_cleanup.remove_floaters`.  Returns (vertices, faces).  `decimation` says who decimates: None (the default) nobody - a
    `face_decimation` other than -1 below the mesh's face count then raises NotImplementedError (at or above it the reference skips
    the decimation too); "hip": `mesh_decimate.decimate_mesh`, rounds of parallel edge collapses on the mesh's device (not the
    reference's `fast_simplification` schedule: mesh_decimate.py).  `decimate_borders` is its `borders`: "fixed" (the default) never
    moves a border vertex, "collapse" lets an open mesh reach the target too."""
    check_mesh(vertices, faces, "process_mesh")
    if decimation not in (None, "hip"):
        raise ValueError(f"process_mesh: decimation must be None or 'hip', got {decimation!r}")
    if decimate_borders not in ("fixed", "collapse"):
        raise ValueError(f"process_mesh: decimate_borders must be 'fixed' or 'collapse', got {decimate_borders!r}")
    vertices, faces, _, _ = _clean(vertices, faces)
    if face_decimation != -1 and faces.shape[0] > face_decimation:
        if decimation is None:
            raise NotImplementedError(f"process_mesh: face_decimation={face_decimation} asks for quadric decimation of a mesh of "
                                      f"{faces.shape[0]} faces; pass decimation='hip' for it, or face_decimation=-1")
        from . import mesh_decimate
        vertices, faces = mesh_decimate.decimate_mesh(vertices, faces, target_faces=face_decimation, borders=decimate_borders)
    if floaters_threshold > 0.0:
        vertices, faces = mesh_cleanup.remove_floaters(vertices, faces, threshold=floaters_threshold)
    return vertices, faces


def expand_to_original(vertices: torch.Tensor, vertex_merge_map: torch.Tensor) -> torch.Tensor:
    """(..., V_merged, 3) -> (..., V_original, 3): every original vertex takes the position of the merged vertex it maps to, so the
    animation fits `pre_merge_faces` (and the UVs that go with them) again."""
    return vertices[..., vertex_merge_map.to(vertices.device), :]


# ---- normalisation --------------------------------------------------------------------------------------------------------------------
@dataclass
class NormalizationParams:
    """What `normalize_mesh` applied.  Tensors on the vertices' device and of their dtype (so nothing is read back): `bbox_center`
    (3,) or None, `scale` 0-d - the largest extent; 0 for a mesh without extent, which is left unscaled."""
    bbox_center: Optional[torch.Tensor]
    scale: torch.Tensor


def normalize_mesh(vertices: torch.Tensor, center: bool = True):
    """Scale (V, 3) vertices into the [-1, 1]^3 cube: bbox_center = (min + max) / 2.0 is subtracted (with `center`), then the
    vertices are multiplied by 2.0 / scale with scale = max extent, when scale > 0.  Min, max and extent in the vertices' dtype.
    Returns (vertices, NormalizationParams); the input is not modified."""
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.shape[0] < 1 or not vertices.is_floating_point():
        raise ValueError(f"normalize_mesh: expected non-empty floating-point (V, 3) vertices, got {tuple(vertices.shape)}")
    bbox_center = None
    if center:
        bbox_center = (vertices.amin(0) + vertices.amax(0)) / 2.0
        vertices = vertices - bbox_center
    scale = (vertices.amax(0) - vertices.amin(0)).amax()
    vertices = vertices * torch.where(scale > 0, 2.0 / scale, torch.ones_like(scale))
    return vertices, NormalizationParams(bbox_center=bbox_center, scale=scale)


def denormalize_mesh(vertices: torch.Tensor, params: NormalizationParams) -> torch.Tensor:
    """Revert `normalize_mesh` on (V, 3) or (T, V, 3) vertices: times scale / 2.0 when scale > 0, plus bbox_center."""
    scale = torch.as_tensor(params.scale, dtype=vertices.dtype, device=vertices.device)
    vertices = vertices * torch.where(scale > 0, scale / 2.0, torch.ones_like(scale))
    if params.bbox_center is not None:
        vertices = vertices + torch.as_tensor(params.bbox_center, dtype=vertices.dtype, device=vertices.device)
    return vertices


def normalize_mesh_to_bounds(vertices: torch.Tensor, bounds: Sequence[float] = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)) -> torch.Tensor:
    """Rescale (V, 3) vertices only if their bounding box exceeds `bounds` = (min_x, min_y, min_z, max_x, max_y, max_z): uniformly by
    min(1, min(target size / max(mesh size, 1e-8))) about the box centre, onto the target centre.  A mesh inside the bounds comes
    back bit for bit (a select on the device: nothing is read back)."""
    b = torch.as_tensor(bounds, dtype=vertices.dtype, device=vertices.device)
    target_min, target_max = b[:3], b[3:]
    flat = vertices.reshape(-1, 3)
    mesh_min, mesh_max = flat.amin(0), flat.amax(0)
    inside = (mesh_min >= target_min).all() & (mesh_max <= target_max).all()
    scale = ((target_max - target_min) / (mesh_max - mesh_min).clamp_min(1e-8)).amin().clamp_max(1.0)
    moved = (vertices - (mesh_min + mesh_max) / 2) * scale + (target_min + target_max) / 2
    return torch.where(inside, vertices, moved)


# ---- surface samples ------------------------------------------------------------------------------------------------------------------
def draw_uniforms(n_points: int, seed: Optional[int] = 0):
    """The uniforms of one `sample_surface` call, drawn on the host exactly as trimesh draws them: `random = default_rng(seed).random`
    (`np.random.random` with seed None), then `random(n)` for the faces and `random((n, 2, 1))` for the barycentric pairs.
    Returns fp64 arrays (n,), (n, 2)."""
    random = np.random.random if seed is None else np.random.default_rng(seed).random
    u_face = random(n_points)
    u_bary = random((n_points, 2, 1))
    return u_face, u_bary.reshape(n_points, 2)


def sample_surface(vertices: torch.Tensor, faces: torch.Tensor, n_points: int, seed: Optional[int] = 0, with_normals: bool = True,
                   device=None, dtype=None, return_face_index: bool = False):
    """Sample `n_points` on the surface of a mesh, uniformly with respect to area: (1, n_points, 3|6) = point | unit normal of its
    face, fp64 unless `dtype` says otherwise, on the vertices' device unless `device` does.  The face areas, the pick (a binary search
    of the area prefix sum) and the points are HIP (am_face_areas, am_surface_sample); the prefix sum is torch.cumsum in fp64; the
    3 n uniforms are `draw_uniforms(n_points, seed)`, uploaded once.  With `return_face_index` also (face indices (n,) int32, the
    prefix sum (F,) fp64)."""
    check_mesh(vertices, faces, "sample_surface")
    faces32 = faces.to(torch.int32).contiguous()
    vertices = vertices.contiguous()
    cdf = torch.cumsum(ops.face_areas(vertices, faces32), 0)
    u_face, u_bary = draw_uniforms(int(n_points), seed)
    u = torch.from_numpy(np.concatenate((u_face, u_bary.reshape(-1)))).to(vertices.device)
    points, face_index, normals = ops.surface_sample(vertices, faces32, cdf, u[:n_points], u[n_points:].view(n_points, 2),
                                                     with_normals=with_normals)
    surface = torch.cat((points, normals), dim=-1) if with_normals else points
    surface = surface.unsqueeze(0)
    if dtype is not None:
        surface = surface.to(dtype)
    if device is not None:
        surface = surface.to(device)
    return (surface, face_index, cdf) if return_face_index else surface
