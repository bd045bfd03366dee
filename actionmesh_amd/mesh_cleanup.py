"""Floater removal on tensors: the reference's `remove_floaters` (actionmesh/preprocessing/mesh_processor.py:288-325), which splits a
`trimesh.Trimesh` into connected components and keeps those with at least `int(max_faces * threshold)` faces, on the
`(vertices, faces)` tensors the Stage-II path here already works on.  The component search is the HIP graph labelling
(`ops.graph_components`, csrc/am_components.hip); the adjacency and the re-indexing are torch plumbing on the same device.

trimesh is not installable where this was written, so two things are a recollection of its behaviour and UNPINNED: the adjacency
rule (`face_adjacency`) and the order in which `trimesh.util.concatenate` lays out the kept components (`remove_floaters`).
What the tests hold is the contract written here, against a brute-force edge dictionary and scipy's connected components.
"""
from __future__ import annotations

import torch

from . import ops
from .mesh_topology import EdgeTables, check_faces, referenced_vertices


def face_adjacency(faces: torch.Tensor) -> torch.Tensor:
    """Pairs of faces that share an undirected edge: int64 (A, 2) on the faces' device, each pair with the lower face first, the
    pairs in the order of their edge (lower vertex, then higher vertex).
    Contract (a recollection of trimesh's `face_adjacency`, UNPINNED): an edge contributes a pair only when EXACTLY two faces use
    it.  A boundary edge (one face) contributes none, and neither does an edge used by three or more faces - so three faces that
    meet in one edge are NOT joined through it."""
    check_faces(faces, "face_adjacency")
    tables = EdgeTables(faces, None, with_order=True)   # no vertex count here, and no read to get one
    counts = tables.edge_count.long()
    first = (torch.cumsum(counts, 0) - counts)[counts == 2]
    return torch.stack((tables.order[first] // 3, tables.order[first + 1] // 3), dim=1)        # half-edge 3 * face + k


def face_components(faces: torch.Tensor):
    """(label, size), int32 (F,) each: the smallest face index of the face's component, and the number of faces in it.  Components
    are those of the `face_adjacency` graph."""
    check_faces(faces, "face_components")
    adj = face_adjacency(faces).to(torch.int32).contiguous()
    return ops.graph_components(faces.shape[0], adj, return_size=True)


def remove_floaters(vertices: torch.Tensor, faces: torch.Tensor, threshold: float = 0.0, return_index: bool = False):
    """Remove small disconnected components from a mesh given as tensors.  vertices (V, 3) or (T, V, 3) - every frame of an animated
    mesh shares the faces and so the kept set - and faces (F, 3).  As the reference: with one component or fewer the INPUT is
    returned; min_faces = int(max_faces * threshold) in Python float arithmetic; components with size >= min_faces are kept; if none
    would be kept the input is returned.
    Order of the result: kept faces stay in their original order, and the vertices they reference stay in their original order,
    re-indexed - a permutation of what `trimesh.util.concatenate` yields (component after component; UNPINNED), which nothing
    downstream depends on.  Vertices no kept face references are dropped, as `mesh.split` drops them.
    Returns (vertices, faces), and with `return_index` also (kept vertex indices, kept face indices), int64."""
    check_faces(faces, "remove_floaters")
    if vertices.dim() not in (2, 3) or vertices.shape[-1] != 3:
        raise ValueError(f"remove_floaters: expected (V, 3) or (T, V, 3) vertices, got {tuple(vertices.shape)}")
    V, F = vertices.shape[-2], faces.shape[0]
    dev = faces.device

    def unchanged():
        if return_index:
            return vertices, faces, torch.arange(V, device=dev), torch.arange(F, device=dev)
        return vertices, faces

    if F == 0:
        return unchanged()
    label, size = face_components(faces)
    is_root = label == torch.arange(F, device=dev, dtype=label.dtype)
    n_components, max_faces = (int(v) for v in torch.stack((is_root.sum(), size.max())).tolist())       # one read
    if n_components <= 1:
        return unchanged()
    min_faces = int(max_faces * threshold)
    keep = size >= min_faces
    if not bool(keep.any()):                    # only with threshold > 1: the largest component always meets threshold <= 1
        return unchanged()
    face_index = torch.nonzero(keep).reshape(-1)
    kept = faces[face_index].long()
    used, remap = referenced_vertices(kept, V)
    vertex_index = torch.nonzero(used).reshape(-1)
    new_faces = remap[kept].to(faces.dtype)
    new_vertices = vertices.index_select(vertices.dim() - 2, vertex_index.to(vertices.device))
    if return_index:
        return new_vertices, new_faces, vertex_index, face_index
    return new_vertices, new_faces
