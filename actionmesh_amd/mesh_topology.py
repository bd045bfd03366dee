"""What the mesh stages know of a face array, stated once: the argument checks, the vertex -> corner CSR (`MeshTopology`), the unique
undirected edges (`EdgeTables`) and the re-numbering of the vertices that faces reference.  Torch only, on the faces' device (it
also runs on CPU tensors); nothing here launches a kernel of this package, so every mesh module and `ops` may import it.
"""
from __future__ import annotations

from typing import Optional

import torch


def check_faces(faces: torch.Tensor, what: str) -> None:
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{what}: expected (F, 3) faces, got {tuple(getattr(faces, 'shape', ()))}")
    if faces.is_floating_point() or faces.dtype == torch.bool:
        raise TypeError(f"{what}: faces must hold integers, got {faces.dtype}")


def check_mesh(vertices: torch.Tensor, faces: torch.Tensor, what: str) -> None:
    check_faces(faces, what)
    if (not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.shape[0] < 1
            or not vertices.is_floating_point()):
        raise ValueError(f"{what}: expected non-empty floating-point (V, 3) vertices, got {tuple(getattr(vertices, 'shape', ()))}")
    if faces.device != vertices.device:
        raise ValueError(f"{what}: vertices on {vertices.device}, faces on {faces.device}")


class MeshTopology:
    """The vertex -> corner CSR of a face array, in the order am_vertex_normals sums in (include/actionmesh_amd.h): corner id
    3 * face + k names vertex faces[face][k]; `corners[offsets[v] : offsets[v + 1]]` are the corners of vertex v in ascending corner
    id.  One stable sort of the flattened faces.  The faces of an animation never change, so one object serves every frame and
    every window.  Indices outside [0, n_vertices) are left out of every vertex's list (the kernel reports them), so building never
    reads the device back."""

    def __init__(self, faces: torch.Tensor, n_vertices: int):
        check_faces(faces, "MeshTopology")
        self.n_vertices, self.n_faces = int(n_vertices), int(faces.shape[0])
        if self.n_vertices < 1:
            raise ValueError(f"MeshTopology: n_vertices {n_vertices} is not positive")
        self.faces = faces.to(torch.int32).contiguous()
        flat, order = torch.sort(self.faces.reshape(-1), stable=True)
        bounds = torch.arange(self.n_vertices + 1, device=faces.device, dtype=torch.int32)
        self.offsets = torch.searchsorted(flat, bounds, out_int32=True).contiguous()
        self.corners = order.to(torch.int32).contiguous()


class EdgeTables:
    """The unique undirected edges of a face array: `edges` (E, 2) int32 with u < v in ascending (u, v), `half_edge_to_edge` (3 F,)
    int32 - half-edge 3 f + k runs from faces[f][k] to faces[f][(k + 1) % 3] - and `edge_count` (E,) int32, the number of half-edges
    of every edge.  One sort of the 3 F keys u * n_vertices + v; without a vertex count (None) the keys are u * 2^32 + v, which
    orders any int32 indices alike.
    `with_order` adds `order` (3 F,) int64: the half-edge ids sorted by edge, ascending within an edge, so the half-edges of edge e
    are `order[first[e] : first[e] + edge_count[e]]` with `first` the exclusive prefix sum of the counts.  The one sort is then a
    stable `torch.sort` in front of `unique_consecutive`, and the half-edge -> edge map is scattered back through `order`; without it
    the sort is `torch.unique`'s own: the decimator builds the tables once a round, a round is about a millisecond on the MI355X,
    and `decimate_mesh` was measured 4 to 12 % slower there with the three-call form.  The three tables are the same either way."""

    def __init__(self, faces: torch.Tensor, n_vertices: Optional[int], with_order: bool = False):
        base = 1 << 32 if n_vertices is None else int(n_vertices)
        f = faces.long()
        a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
        key = torch.minimum(a, b) * base + torch.maximum(a, b)
        self.order = None
        if with_order:
            key, self.order = torch.sort(key, stable=True)
            uniq, inverse, counts = torch.unique_consecutive(key, return_inverse=True, return_counts=True)
            inverse = torch.empty_like(inverse).index_copy_(0, self.order, inverse)
        else:
            uniq, inverse, counts = torch.unique(key, return_inverse=True, return_counts=True)
        self.edges = torch.stack((uniq // base, uniq % base), dim=1).to(torch.int32).contiguous()
        self.half_edge_to_edge = inverse.to(torch.int32).contiguous()
        self.edge_count = counts.to(torch.int32).contiguous()


def _rank(keep: torch.Tensor) -> torch.Tensor:
    """The position of every kept entry among the kept ones, int64; what a dropped entry gets is the rank of the last kept one
    before it (-1 in front of the first)."""
    return torch.cumsum(keep, 0) - 1


def referenced_vertices(faces: torch.Tensor, n_vertices: int):
    """(used (n_vertices,) bool: some face names the vertex; rank (n_vertices,) int64: the new index of every used vertex when the
    unused ones are dropped and the others keep their order).  The indices must lie inside [0, n_vertices)."""
    used = torch.zeros((n_vertices,), dtype=torch.bool, device=faces.device)
    used[faces.reshape(-1).long()] = True
    return used, _rank(used)


def compact_rows(rows: torch.Tensor, keep: torch.Tensor, n_keep: int) -> torch.Tensor:
    """The rows with `keep` set, in order, as a fresh tensor of n_keep rows, without reading the device: every row is written to its
    rank among the kept ones, a dropped one (or one beyond n_keep) to a spare row that is cut off."""
    rank = _rank(keep)
    dest = torch.where(keep & (rank < n_keep), rank, torch.full_like(rank, n_keep))
    out = torch.empty((n_keep + 1,) + tuple(rows.shape[1:]), dtype=rows.dtype, device=rows.device)
    out.index_copy_(0, dest, rows)
    return out[:n_keep].contiguous()
