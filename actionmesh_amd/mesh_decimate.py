"""Mesh decimation on tensors: `decimate_mesh`, the reference's `MeshPostprocessor` step that brings every Stage-0 mesh down to
`face_decimation` faces (actionmesh/preprocessing/mesh_processor.py:128-161, through `trimesh.simplify_quadric_decimation` and
`fast_simplification`), as rounds of independent quadric edge collapses.  A sequential priority queue does not map to a GPU; a
round here evaluates every edge at once, picks a set of edges whose closed stars share no face, and collapses them all:

  per mesh   quadrics: every vertex sums the area-weighted plane quadrics of its faces                       ops.decimate_quadrics
  per round  1. torch plumbing on the mesh's device (it also runs on CPU tensors): the vertex -> corner CSR of the live faces
                (`mesh_topology.MeshTopology`) and their unique undirected edges (`mesh_topology.EdgeTables`) - one `torch.unique`
                (a sort) of the 3 F half-edge keys, with the inverse (half-edge -> edge) and the use count of every edge;
             2. every edge gets a candidate position, a cost and a 64-bit key (cost as fp32 bits, then a bijective hash of the
                edge index), or "not a candidate" when an endpoint is on a border or a non-manifold edge, the link condition
                fails, or a face of either star would flip or degenerate                                      ops.decimate_edges
             3. an edge is selected when its key is the smallest among all edges within one edge of either endpoint (two
                gathers, no atomics): selected edges have neither equal nor adjacent endpoints                ops.decimate_select
             4. if all of them would undershoot the target, only the ceil((F - target) / 2) smallest keys are kept (one sort);
             5. the kept edges collapse in place, u <- v with u < v: new position, summed quadrics, v's corners renamed, the
                edge's two faces dropped                                                                      ops.decimate_apply
The arithmetic of the four kernels is written out in include/actionmesh_amd.h (csrc/am_decimate.hip); it is fp64 without fused
multiply-adds and without floating-point atomics, so the result is the same bits on every run and equals a numpy restatement of
the header (tests/test_mesh_decimate_*).  Every permitted collapse removes exactly two faces, so a mesh that reaches the target ends
with `target_faces` or `target_faces - 1` faces.  A round that selects nothing ends the loop: the mesh comes back with more faces
than asked and a logged warning, not an exception (two glued tetrahedra and a mesh that is all border are such inputs).

BORDERS.  `borders="fixed"` (the default) is the scheme above and its bits: border vertices never move.  `borders="collapse"` lets
open meshes reach the target (the header's "Border collapses"): vertices are interior, border or locked; border vertices slide along
their border loop and border edges collapse, under the link condition of the surface closed by a cone over its borders; every
border half-edge adds one constraint plane (through the edge, perpendicular to its face, weight `border_weight` * |edge|^2) to
the quadrics of its two ends.                                                 ops.decimate_border_quadrics, ops.decimate_border_edges
The edge tables are then built before the quadrics; selection and apply are the same kernels.  A collapse removes edge_count faces,
1 or 2, so step 4 becomes: among the selected edges in ascending key order keep the shortest prefix whose removed faces reach
F - target (or all of them) - one sort and one cumulative sum of edge_count on the device, and the mesh still ends with
`target_faces` or `target_faces - 1` faces when they can be reached.  On a mesh without border the two modes give the same bits.
`border_weight`'s default 1.0 makes leaving the border curve by a distance cost about what leaving the surface by it does (a face
plane weighs about 0.43 L^2 and an interior vertex sums 5 to 6 of them; a border vertex sums two border planes of L^2): a
plausible scale, nothing stronger.

The kernel calls go through one small backend object (`HipBackend`), so the tests can run the same loop on CPU tensors with a numpy
restatement in its place.  No CPU backend is shipped.

Device-to-host reads: one for the quadrics' flag, then ONE per round - the flag words of the round's kernels together with the
number of selected edges, which sizes the apply launch and, as every collapse removes two faces, gives the next face count (with
`borders="collapse"`: the number of kept edges and the number of faces they remove).

UNPINNED: parity with `fast_simplification` is not attempted.  That library collapses sequentially by a dirty-flag threshold
schedule and uses unweighted planes; this one uses area-weighted planes and the round schedule above.  What is pinned is the
header's contract, the invariants (manifoldness, Euler characteristic, no flipped or degenerate face) and the surface distance
against a sequential greedy decimation with the same cost (profiles/mesh_decimate.json; with border collapses also the distance of
the border curves, profiles/mesh_decimate_borders.json).
"""
from __future__ import annotations

import logging
import math
from typing import Optional

import torch

from . import _lib as L
from . import ops
from .mesh_topology import EdgeTables, MeshTopology, check_mesh, compact_rows, referenced_vertices

logger = logging.getLogger(__name__)

NO_KEY = L.DECIMATE_NO_KEY
MAX_ROUNDS = 4096               # far above what any mesh needs (tens): a guard against a loop that cannot end


class HipBackend:
    """The four kernels of a round (csrc/am_decimate.hip), and the two that replace the first two with `borders="collapse"`.  `flag`:
    the caller's int32 (1,) word, which it reads with the round's other figures; quadrics reads its own."""

    quadrics = staticmethod(ops.decimate_quadrics)
    edges = staticmethod(ops.decimate_edges)
    select = staticmethod(ops.decimate_select)
    apply = staticmethod(ops.decimate_apply)
    border_quadrics = staticmethod(ops.decimate_border_quadrics)
    border_edges = staticmethod(ops.decimate_border_edges)


def _check_borders(borders: str, border_weight: float) -> float:
    if borders not in ("fixed", "collapse"):
        raise ValueError(f"decimate_mesh: borders must be 'fixed' or 'collapse', got {borders!r}")
    try:
        weight = float(border_weight)
    except (TypeError, ValueError):
        raise ValueError(f"decimate_mesh: border_weight {border_weight!r} is not a number") from None
    if not (math.isfinite(weight) and weight >= 0.0):
        raise ValueError(f"decimate_mesh: border_weight {border_weight!r} is not finite and >= 0")
    return weight


def _by_key(selected: torch.Tensor, key: torch.Tensor) -> torch.Tensor:
    """The edge indices with the selected edges first, the smallest keys first (one sort on the device)."""
    return torch.sort(torch.where(selected != 0, key, torch.full_like(key, NO_KEY))).indices


def decimate_rounds(positions: torch.Tensor, faces: torch.Tensor, target_faces: int, backend=None, observer=None, borders: str = "fixed",
                    border_weight: float = 1.0):
    """The round loop on fp64 positions (V, 3) and int32 faces (F, 3), both contiguous.  Returns (positions (V, 3) fp64 - the
    original vertex numbering, moved vertices in place -, live faces (F', 3) int32, vertex map (V,) int64: every vertex to the one
    it was merged into, rounds run).  `observer(round, state dict)` is called after every selection (tests); with
    `borders="collapse"` the dict also holds `kept`, the edges the round collapses."""
    border_weight = _check_borders(borders, border_weight)
    collapse = borders == "collapse"
    backend = HipBackend if backend is None else backend
    V, dev = positions.shape[0], positions.device
    positions, faces = positions.clone(), faces.clone()
    topology = MeshTopology(faces, V)
    tables = None
    if collapse:
        tables = EdgeTables(faces, V)
        quadrics = backend.border_quadrics(positions, faces, topology, tables.half_edge_to_edge, tables.edge_count, border_weight)
    else:
        quadrics = backend.quadrics(positions, faces, topology)
    evaluate = backend.border_edges if collapse else backend.edges
    merged = torch.arange(V, device=dev)
    flags = torch.zeros((3,), dtype=torch.int32, device=dev)           # edges, select, apply (the last round's)
    rounds = 0
    while faces.shape[0] > target_faces and rounds < MAX_ROUNDS:
        F = faces.shape[0]
        if rounds:
            topology = MeshTopology(faces, V)
        if rounds or tables is None:
            tables = EdgeTables(faces, V)
        cand, cost, key = evaluate(positions, quadrics, faces, topology, tables.edges, tables.half_edge_to_edge, tables.edge_count,
                                   flag=flags[0:1])
        m1, m2, selected = backend.select(V, faces, topology, tables.edges, tables.half_edge_to_edge, key, flag=flags[1:2])
        state = dict(positions=positions, quadrics=quadrics, faces=faces, topology=topology, tables=tables, candidates=cand, cost=cost,
                     key=key, m1=m1, m2=m2, selected=selected)
        if collapse:
            # the shortest prefix, in key order, of the selected edges whose faces (1 or 2 each) reach F - target: on the device
            order = _by_key(selected, key)
            removed = torch.cumsum(torch.where(selected[order] != 0, tables.edge_count[order].long(), 0), 0)
            n_kept = torch.minimum((removed < F - target_faces).sum() + 1, (selected != 0).sum())
            n_removed = removed[torch.clamp(n_kept - 1, min=0)] * (n_kept > 0)
            f_edges, f_select, f_apply, n_kept, n_removed = torch.cat((flags.long(), n_kept.reshape(1), n_removed.reshape(1))).tolist()
            n_selected = n_kept                                                                                   # the round's one read
            state["kept"] = order[:n_kept]
        else:
            f_edges, f_select, f_apply, n_selected = torch.cat((flags.long(), selected.sum().reshape(1))).tolist()     # the round's one read
        if f_edges | f_select | f_apply:
            raise ValueError("decimate_mesh: " + ops.decimate_flag_message(f_edges | f_select | f_apply, V))
        if observer is not None:
            observer(rounds, state)
        if n_selected == 0:
            logger.warning("decimate_mesh: no edge can collapse any more; the mesh keeps %d faces, %d were asked for", F, target_faces)
            break
        if collapse:
            kept = state["kept"].to(torch.int32).contiguous()
        else:
            n_kept = min(n_selected, (F - target_faces + 1) // 2)
            n_removed = 2 * n_kept
            kept = _by_key(selected, key)[:n_kept].to(torch.int32).contiguous()
        round_map = torch.arange(V, device=dev, dtype=torch.int32)
        dead = backend.apply(positions, quadrics, faces, topology, tables.edges, cand, kept, round_map, flag=flags[2:3])
        merged = round_map.long()[merged]
        faces = compact_rows(faces, dead == 0, F - n_removed)
        rounds += 1
    bits = int(flags[2])
    if bits:
        raise ValueError("decimate_mesh: " + ops.decimate_flag_message(bits, V))
    return positions, faces, merged, rounds


def decimate_mesh(vertices: torch.Tensor, faces: torch.Tensor, target_faces: int = 40_000, return_map: bool = False, backend=None,
                  return_rounds: bool = False, borders: str = "fixed", border_weight: float = 1.0):
    """Decimate a mesh to `target_faces` faces by quadric edge collapse (the module docstring has the algorithm).  vertices (V, 3)
    floating point, faces (F, 3) integer, on one device.  As the reference, a mesh with `target_faces` faces or fewer comes back
    as it is - the same tensors.  Otherwise returns (vertices', faces') in the input dtypes: surviving vertices in their original
    relative order (an unmoved one keeps its bits), vertices no face references dropped, `target_faces` or `target_faces - 1` faces
    when the target can be reached.  With `borders="fixed"`, border vertices and vertices on non-manifold edges are never moved or
    removed; with `borders="collapse"` border vertices move along their border and border edges collapse (`border_weight`, finite and
    >= 0, scales the border's constraint planes; the module docstring), and only vertices on non-manifold edges or on more than one
    border loop stay locked.  A mesh that runs out of permitted collapses comes back with more faces than asked and a logged
    warning.  With `return_map` also an int64 (V,) map
    in the ORIGINAL numbering from every vertex to the surviving vertex it was merged into (survivors map to themselves:
    `map[map] == map`, and `vertices'` are the final positions of the referenced fixed points, in order); with `return_rounds` the
    number of rounds run.  A face index outside [0, V) raises ValueError.  `backend`: the kernels (tests)."""
    check_mesh(vertices, faces, "decimate_mesh")
    border_weight = _check_borders(borders, border_weight)
    target_faces = int(target_faces)
    if target_faces < 0:
        raise ValueError(f"decimate_mesh: target_faces {target_faces} is negative")
    V, dev = vertices.shape[0], vertices.device
    if faces.shape[0] <= target_faces:
        out = (vertices, faces)
        rounds = 0
        merged = torch.arange(V, device=dev) if return_map else None
    else:
        positions, live, merged, rounds = decimate_rounds(vertices.double().contiguous(), faces.to(torch.int32).contiguous(), target_faces,
                                                          backend=backend, borders=borders, border_weight=border_weight)
        used, remap = referenced_vertices(live, V)
        out = (positions[used].to(vertices.dtype), remap[live.long()].to(faces.dtype))
    if return_map:
        out = out + (merged,)
    if return_rounds:
        out = out + (rounds,)
    return out
