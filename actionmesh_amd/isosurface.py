"""Iso-surface extraction on tensors (INTEGRATION seam S11): the step that turns the Stage-0 VAE's field into the anchor mesh.  The
reference reaches it through TripoSG's `hierarchical_extract_geometry` (actionmesh/external/triposg.py:13, 193-199), which runs the
`diso` package's dual marching cubes - a CUDA-only wheel that does not build for ROCm.  Here it is marching tetrahedra on the regular
grid: every cell is cut into the six Kuhn tetrahedra, whose diagonals agree between neighbouring cells, so the output is always a
combinatorial 2-manifold with one orientation (closed wherever the surface stays inside the evaluated points) - which is what
`decimate_mesh`, the next step, needs: it never touches a non-manifold vertex.

  ops.iso_classify    per point the mask of crossing edges that start there, per cell the number of triangles
  torch plumbing      the two exclusive prefix sums (`torch.cumsum`, int64) and ONE device-to-host read of their totals, which
                      sizes the outputs
  ops.iso_vertices    every crossing edge's vertex at its rank: one vertex per edge, in ascending edge id
  ops.iso_triangles   every cell's triangles at its offset: ordered by cell, tetrahedron, triangle
  torch plumbing      vertices that no face uses (crossing edges next to non-finite samples) are dropped, order preserved; ONE
                      more read: the two kernels' flag words with the number of vertices kept
The arithmetic is written out in include/actionmesh_amd.h (csrc/am_isosurface.hip): fp64 interpolation without fused multiply-adds,
no atomics, no hash table - the same bits on every run, equal to a numpy restatement of the header (tests/test_isosurface_*).  The
kernel calls go through one small backend object (`HipBackend`), so the tests can run the same code on CPU tensors with that
restatement in its place.  No CPU backend is shipped.

`method="dual"` (opt-in; the default stays "tetrahedra") is the second extraction: dual marching cubes with a manifold rule, over
csrc/am_dualcubes.hip - one vertex per patch of every active cell, one quad per crossing grid edge, about a third of the triangles,
with the same guarantees (a closed, oriented 2-manifold wherever the surface stays inside the evaluated points; the same bits on every
run) and the same shape of the call:
  ops.dmc_cells       per cell its configuration (the 8-bit inside mask; 0 unless all eight corners are finite and not on one side)
                      and which of its faces is "double"
  ops.dmc_classify    per cell its code - configuration, + 256 when its double face is double in the neighbour too and therefore
                      flipped, which is what keeps the mesh a manifold -, its number of patches, and per point the mask of the axis
                      edges that emit a quad
  torch plumbing      the two prefix sums and the ONE sizing read, as above
  ops.dmc_vertices    every patch's vertex - the mean of its edges' crossings, fp64, rounded once - at its cell's offset + patch
  ops.dmc_triangles   every emitting edge's quad, split along its shorter diagonal, at its offset
  torch plumbing      unused vertices (next to non-finite samples or the grid border) dropped; the second and last read
Its kernels go through a second backend object (`HipDualBackend`, keyword `dual_backend`).

`hierarchical_extract_geometry` has the reference call site's name and keywords: a dense grid of 2^dense + 1 points per axis, then for
every further depth only the 3 x 3 x 3 fine points of the cells the surface passes through (dilated), everything else NaN - "not
evaluated" - and the extraction at the finest depth.

UNPINNED: parity with `diso` (its vertex placement, its diagonal rule, its tables) or with skimage is not attempted, by either
method - neither can be installed where this was written; sharp-feature (QEF) vertex placement is not attempted: a dual vertex is the
mean of its patch's crossings; TripoSG's refinement schedule and its `flash_extract_geometry` variant are not reproduced, the
schedule here is this project's own; the sign convention of the VAE's field is an assumption: positive inside by default,
`inside="below"` for the other.  What is pinned is the header's contract and the invariants (every edge in two faces, every directed
edge once, the Euler characteristic, the enclosed volume).
"""
from __future__ import annotations

import logging
from typing import Optional, Sequence

import numpy as np
import torch

from . import ops
from .mesh_topology import EdgeTables, compact_rows, referenced_vertices

logger = logging.getLogger(__name__)

MAX_ITEMS = 2 ** 31 - 1
DEFAULT_BOUNDS = (-1.005, -1.005, -1.005, 1.005, 1.005, 1.005)
_POPCOUNT = [bin(i).count("1") for i in range(256)]


class HipBackend:
    """The three kernels (csrc/am_isosurface.hip).  `flag`: the caller's int32 (1,) word, which it reads with its other figures."""

    classify = staticmethod(ops.iso_classify)
    vertices = staticmethod(ops.iso_vertices)
    triangles = staticmethod(ops.iso_triangles)


class HipDualBackend:
    """The four kernels of method="dual" (csrc/am_dualcubes.hip).  `flag` as in HipBackend."""

    cells = staticmethod(ops.dmc_cells)
    classify = staticmethod(ops.dmc_classify)
    vertices = staticmethod(ops.dmc_vertices)
    triangles = staticmethod(ops.dmc_triangles)


METHODS = ("tetrahedra", "dual")


def _method(who: str, method) -> str:
    if method not in METHODS:
        raise ValueError(f"{who}: method must be 'tetrahedra' or 'dual', got {method!r}")
    return method


def _inside_above(inside) -> bool:
    if inside not in ("above", "below"):
        raise ValueError(f"extract_isosurface: inside must be 'above' or 'below', got {inside!r}")
    return inside == "above"


def _bounds(who: str, bounds) -> list:
    """The box (x0, y0, z0, x1, y1, z1) as six floats; one number b means (-b, -b, -b, b, b, b)."""
    b = [float(x) for x in ((-bounds,) * 3 + (bounds,) * 3 if isinstance(bounds, (int, float)) else bounds)]
    if len(b) != 6:
        raise ValueError(f"{who}: bounds are (x0, y0, z0, x1, y1, z1), got {len(b)} numbers")
    return b


def _frame(shape, bounds, origin, spacing):
    """(origin, spacing) as two tuples of three floats: given directly, or from bounds (x0, y0, z0, x1, y1, z1) - the first and the
    last point of every axis -, or the index frame."""
    if bounds is not None:
        if origin is not None or spacing is not None:
            raise ValueError("extract_isosurface: give bounds or origin / spacing, not both")
        b = _bounds("extract_isosurface", bounds)
        return tuple(b[:3]), tuple((b[3 + c] - b[c]) / (shape[c] - 1) for c in range(3))
    origin = (0.0, 0.0, 0.0) if origin is None else tuple(float(x) for x in origin)
    spacing = (1.0, 1.0, 1.0) if spacing is None else tuple(float(x) for x in spacing)
    if len(origin) != 3 or len(spacing) != 3:
        raise ValueError("extract_isosurface: origin and spacing are three numbers each")
    return origin, spacing


def _empty(dev):
    return torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.int64, device=dev)


def _sized(vertex_counts: torch.Tensor, tri_counts: torch.Tensor, shape):
    """The middle of both methods, from the flat per-point numbers of vertices and of triangles (integers; summed in int64): the two
    prefix sums and the ONE read of their totals; more than MAX_ITEMS of either raises.  None where the surface does not cross the grid,
    else (n_vertices, n_triangles, the two exclusive offsets as int64 `shape`, the (2,) int32 flag words of the kernels that follow)."""
    vertex_end, tri_end = torch.cumsum(vertex_counts, 0, dtype=torch.int64), torch.cumsum(tri_counts, 0, dtype=torch.int64)
    n_vertices, n_triangles = torch.stack((vertex_end[-1], tri_end[-1])).tolist()              # the read that sizes the outputs
    if n_vertices > MAX_ITEMS or n_triangles > MAX_ITEMS:
        raise ValueError(f"extract_isosurface: {n_vertices} vertices and {n_triangles} triangles; more than 2^31 - 1 of either is "
                         "not supported")
    if n_vertices == 0 or n_triangles == 0:
        return None
    flags = torch.zeros((2,), dtype=torch.int32, device=vertex_counts.device)
    return n_vertices, n_triangles, (vertex_end - vertex_counts).view(shape), (tri_end - tri_counts).view(shape), flags


def _used_vertices_only(vertices, faces, flags, n_vertices: int, flag_message):
    """The end of both methods: the vertices that no face uses dropped, order preserved, with the second and last device-to-host
    read - the two kernels' flag words and the number of vertices kept; a set flag bit raises."""
    # a valid face index lies inside [0, n_vertices); where a flag is set a row may be unwritten, so the scatter below is clamped
    used, rank = referenced_vertices(faces.long().clamp_(0, n_vertices - 1), n_vertices)
    f_vertices, f_triangles, n_used = torch.cat((flags.long(), rank[-1:] + 1)).tolist()
    if f_vertices | f_triangles:
        raise ValueError("extract_isosurface: " + flag_message(f_vertices | f_triangles))
    if n_used == n_vertices:
        return vertices, faces.long()
    return compact_rows(vertices, used, n_used), rank[faces.long()]


def extract_isosurface(values: torch.Tensor, level: float = 0.0, bounds=None, origin=None, spacing=None, inside: str = "above",
                       backend=None, method: str = "tetrahedra", dual_backend=None):
    """The surface `values == level` of an fp32 grid (X, Y, Z), every axis at least 2, as (vertices (V, 3) fp32, faces (F, 3) int64)
    on the tensor's device, oriented with the normals from the inside - finite and above the level, or below it with
    `inside="below"` - to the outside.  A non-finite value means "not evaluated": no triangle touches it.  Positions: point (i, j, k)
    lies at origin + (i, j, k) * spacing, given directly or through `bounds` (x0, y0, z0, x1, y1, z1), the positions of the first and
    last points; the index frame without either.  Every returned vertex is used by a face.  A grid the surface does not cross gives
    (0, 3) and (0, 3).  More than 2^31 - 1 vertices or triangles raise ValueError before anything is extracted.  `method`:
    "tetrahedra" (marching tetrahedra) or "dual" (dual marching cubes: about a third of the triangles, the same guarantees).
    `backend`, `dual_backend`: the kernels of the two methods (tests)."""
    method = _method("extract_isosurface", method)
    backend = HipBackend if backend is None else backend
    dual_backend = HipDualBackend if dual_backend is None else dual_backend
    if not isinstance(values, torch.Tensor) or values.dim() != 3 or min(values.shape) < 2:
        raise ValueError(f"extract_isosurface: expected (X, Y, Z) values with every axis at least 2, got {tuple(getattr(values, 'shape', ()))}")
    if values.dtype != torch.float32:
        raise TypeError(f"extract_isosurface: expected float32 values, got {values.dtype}")
    above = _inside_above(inside)
    level = float(level)
    if not np.isfinite(level):
        raise ValueError(f"extract_isosurface: the level must be finite, got {level}")
    origin, spacing = _frame(values.shape, bounds, origin, spacing)
    values, dev = values.contiguous(), values.device
    if method == "dual":
        return _extract_dual(values, level, above, origin, spacing, dual_backend)
    mask, count = backend.classify(values, level, above)
    crossings = torch.tensor(_POPCOUNT, dtype=torch.int64, device=dev)[mask.reshape(-1).long()]
    sized = _sized(crossings, count.reshape(-1), values.shape)
    if sized is None:
        return _empty(dev)
    n_vertices, n_triangles, vertex_offset, tri_offset, flags = sized
    vertices = backend.vertices(values, mask, vertex_offset, n_vertices, origin, spacing, level, flag=flags[0:1])
    faces = backend.triangles(values, mask, count, vertex_offset, tri_offset, n_vertices, n_triangles, level, above, flag=flags[1:2])
    return _used_vertices_only(vertices, faces, flags, n_vertices, ops.iso_flag_message)


def _extract_dual(values: torch.Tensor, level: float, above: bool, origin, spacing, backend):
    """extract_isosurface's method="dual" behind its argument checks: the same two reads, the same limits, the same empty result."""
    dev = values.device
    config, double = backend.cells(values, level, above)
    code, count, edge_mask = backend.classify(config, double)
    triangles = 2 * torch.tensor(_POPCOUNT[:8], dtype=torch.int64, device=dev)[edge_mask.reshape(-1).long().clamp_(max=7)]
    sized = _sized(count.reshape(-1), triangles, values.shape)
    if sized is None:
        return _empty(dev)
    n_vertices, n_triangles, vertex_offset, tri_offset, flags = sized
    vertices = backend.vertices(values, code, vertex_offset, n_vertices, origin, spacing, level, above, flag=flags[0:1])
    faces = backend.triangles(code, edge_mask, vertex_offset, tri_offset, vertices, n_vertices, n_triangles, flag=flags[1:2])
    return _used_vertices_only(vertices, faces, flags, n_vertices, ops.dmc_flag_message)


def border_edge_count(faces: torch.Tensor) -> int:
    """The number of edges that only one face uses (0 on a closed surface).  One sort; one device-to-host read."""
    if faces.shape[0] == 0:
        return 0
    return int((EdgeTables(faces, None).edge_count == 1).sum())


def _axis_points(lo: float, hi: float, n: int, dev) -> torch.Tensor:
    """The n positions of one axis in float32: `np.linspace` in float64 on the host (n is a few hundred), rounded once."""
    return torch.from_numpy(np.linspace(lo, hi, n).astype(np.float32)).to(dev)


def _evaluate(geometric_func, axes, linear: Optional[torch.Tensor], n: int, max_points_per_call: int, dtype) -> torch.Tensor:
    """The field at the points `linear` (indices into the n^3 grid; all of them when None), in chunks: (B, len) float32."""
    dev = axes[0].device
    total = n ** 3 if linear is None else linear.numel()
    out = []
    for start in range(0, total, max_points_per_call):
        idx = torch.arange(start, min(start + max_points_per_call, total), device=dev) if linear is None else linear[start:start + max_points_per_call]
        pts = torch.stack((axes[0][idx // (n * n)], axes[1][(idx // n) % n], axes[2][idx % n]), dim=-1).to(dtype)
        val = geometric_func(pts.unsqueeze(0))
        if val.dim() == 3 and val.shape[-1] == 1:
            val = val[..., 0]
        if val.dim() != 2 or val.shape[1] != idx.numel():
            raise ValueError(f"hierarchical_extract_geometry: geometric_func returned {tuple(val.shape)} for {idx.numel()} points")
        out.append(val.float())
    return torch.cat(out, dim=1)


def hierarchical_extract_geometry(geometric_func, device, bounds=DEFAULT_BOUNDS, dense_octree_depth: int = 8,
                                  hierarchical_octree_depth: int = 9, dilation: int = 1, max_points_per_call: int = 1 << 21,
                                  level: float = 0.0, inside: str = "above", dtype=torch.float32, backend=None,
                                  method: str = "tetrahedra", dual_backend=None):
    """TripoSG's entry point as the reference calls it (triposg.py:193-199): `geometric_func(points (B, n, 3)) -> (B, n, 1)` is the
    field, `bounds` the box (one number b means (-b, -b, -b, b, b, b)).  Returns a list with one (vertices np.float32 (V, 3), faces
    np.int64 (F, 3)) per batch entry of what the function returns.

    The schedule: the grid of 2^dense_octree_depth + 1 points per axis is evaluated whole, `max_points_per_call` points at a time.
    For every further depth up to hierarchical_octree_depth, the active coarse cells - a non-zero triangle count from
    `ops.iso_classify`: eight finite corners, not all on one side - of ANY batch entry are dilated by `dilation` cells, the
    3 x 3 x 3 fine points of each are evaluated, and every other fine point is NaN.  That test is also the ACTIVE of method="dual",
    so the schedule is the same for both methods; `method` chooses the extraction at the finest depth (`extract_isosurface`);
    when it has border edges - it left the evaluated band, or the box - their number is logged as a warning.  The points handed to
    `geometric_func` are `dtype` (float32) on `device`: `np.linspace` between the bounds in float64, rounded once."""
    method = _method("hierarchical_extract_geometry", method)
    backend = HipBackend if backend is None else backend
    above = _inside_above(inside)
    dense, finest = int(dense_octree_depth), max(int(dense_octree_depth), int(hierarchical_octree_depth))
    if dense < 1 or finest > 10:
        raise ValueError(f"hierarchical_extract_geometry: depths {dense} .. {finest} are outside 1 .. 10")
    if int(dilation) < 0 or int(max_points_per_call) < 1:
        raise ValueError("hierarchical_extract_geometry: dilation must be >= 0 and max_points_per_call >= 1")
    b = _bounds("hierarchical_extract_geometry", bounds)
    dev = torch.device(device)
    n = 2 ** dense + 1
    axes = [_axis_points(b[c], b[3 + c], n, dev) for c in range(3)]
    values = _evaluate(geometric_func, axes, None, n, int(max_points_per_call), dtype)
    values = values.reshape(values.shape[0], n, n, n)
    for depth in range(dense + 1, finest + 1):
        active = torch.zeros((n - 1,) * 3, dtype=torch.bool, device=dev)
        for grid in values:
            active |= backend.classify(grid.contiguous(), level, above)[1][:-1, :-1, :-1] != 0
        if int(dilation):
            k = 2 * int(dilation) + 1
            active = torch.nn.functional.max_pool3d(active[None, None].float(), k, stride=1, padding=int(dilation))[0, 0] != 0
        n = 2 ** depth + 1
        cells = torch.nonzero(active)                                     # (K, 3); a read: it sizes the evaluation
        offsets = torch.stack(torch.meshgrid(*(torch.arange(3, device=dev),) * 3, indexing="ij"), dim=-1).reshape(-1, 3)
        fine = (2 * cells[:, None, :] + offsets[None]).reshape(-1, 3)
        marked = torch.zeros((n ** 3,), dtype=torch.bool, device=dev)
        marked[(fine[:, 0] * n + fine[:, 1]) * n + fine[:, 2]] = True
        linear = torch.nonzero(marked)[:, 0]
        axes = [_axis_points(b[c], b[3 + c], n, dev) for c in range(3)]
        next_values = torch.full((values.shape[0], n ** 3), float("nan"), dtype=torch.float32, device=dev)
        if linear.numel():
            next_values[:, linear] = _evaluate(geometric_func, axes, linear, n, int(max_points_per_call), dtype)
        values = next_values.reshape(-1, n, n, n)
    meshes = []
    for grid in values:
        vertices, faces = extract_isosurface(grid, level, bounds=b, inside=inside, backend=backend, method=method, dual_backend=dual_backend)
        borders = border_edge_count(faces)
        if borders:
            logger.warning("hierarchical_extract_geometry: the surface has %d border edges: it left the evaluated band or the bounds",
                           borders)
        meshes.append((vertices.cpu().numpy(), faces.cpu().numpy()))
    return meshes


# ---- seam S11 --------------------------------------------------------------------------------------------------------------------
SEAM_NAME = "hierarchical_extract_geometry"
PIPELINE_MODULE = "triposg.pipelines.pipeline_triposg"
_MISSING = object()


def hierarchical_extract_geometry_dual(*args, **kwargs):
    """`hierarchical_extract_geometry` with method="dual" as its default: what `install_into(module, method="dual")` installs."""
    kwargs.setdefault("method", "dual")
    return hierarchical_extract_geometry(*args, **kwargs)


def install_into(module, method: str = "tetrahedra") -> dict:
    """Give `module` - meant for `actionmesh.external.triposg` - this module's `hierarchical_extract_geometry` (with
    method="dual": `hierarchical_extract_geometry_dual`, the same function with that method as its default) under the name it
    imported from `triposg.inference_utils` (triposg.py:13), which `TripoSGVAE.decode_latents` resolves at call time.  When the
    `triposg` package is importable, the pipeline module that imported the same name (`TripoSGPipeline.__call__`, reached through
    `TripoSGPipelinePlus`) gets it too.  Returns what the names held, for `uninstall_from`."""
    ours = hierarchical_extract_geometry_dual if _method("install_into", method) == "dual" else hierarchical_extract_geometry
    saved = {"module": getattr(module, SEAM_NAME, _MISSING), "pipeline": None}
    setattr(module, SEAM_NAME, ours)
    try:
        import importlib
        pipeline = importlib.import_module(PIPELINE_MODULE)
    except ImportError:
        pipeline = None
    if pipeline is not None and hasattr(pipeline, SEAM_NAME):
        saved["pipeline"] = (pipeline, getattr(pipeline, SEAM_NAME))
        setattr(pipeline, SEAM_NAME, ours)
    return saved


def uninstall_from(module, saved: dict) -> None:
    if saved["module"] is _MISSING:
        if hasattr(module, SEAM_NAME):
            delattr(module, SEAM_NAME)
    else:
        setattr(module, SEAM_NAME, saved["module"])
    if saved.get("pipeline"):
        pipeline, value = saved["pipeline"]
        setattr(pipeline, SEAM_NAME, value)
