"""`actionmesh_amd.mesh_topology` on CPU tensors: `EdgeTables` against a brute-force Python dictionary of the undirected edges, what
`face_adjacency` and `border_edge_count` derive from the tables against the same dictionary, and `referenced_vertices` /
`compact_rows` against `numpy.unique` and boolean indexing."""
import numpy as np
import pytest
import torch

from actionmesh_amd import isosurface, mesh_cleanup, mesh_decimate, mesh_prep
from actionmesh_amd import mesh_topology as MT

N_RANDOM_VERTICES = 7
RANDOM_FACES = np.random.default_rng(11).integers(0, N_RANDOM_VERTICES, (300, 3))      # repeated indices within a face included
TETRAHEDRON = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])

CASES = {
    "one-triangle": (np.array([[0, 1, 2]]), 3),
    "tetrahedron": (TETRAHEDRON, 4),
    "shared-edge-equal-winding": (np.array([[0, 1, 2], [0, 1, 3]]), 4),
    "shared-edge-opposite-winding": (np.array([[0, 1, 2], [1, 0, 3]]), 4),
    "three-on-an-edge": (np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]]), 5),
    "self-edge": (np.array([[0, 1, 2], [3, 3, 1]]), 4),
    "random-7x300": (RANDOM_FACES, N_RANDOM_VERTICES),
}
cases = pytest.mark.parametrize("faces,n_vertices", list(CASES.values()), ids=list(CASES))


def edge_dictionary(faces: np.ndarray) -> dict:
    """(u, v) with u <= v -> the half-edge ids 3 f + k of that undirected edge, ascending."""
    edges = {}
    for f, tri in enumerate(faces.tolist()):
        for k in range(3):
            a, b = tri[k], tri[(k + 1) % 3]
            edges.setdefault((min(a, b), max(a, b)), []).append(3 * f + k)
    return edges


@cases
@pytest.mark.parametrize("known_count", [True, False], ids=["n_vertices", "no-vertex-count"])
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_edge_tables_against_the_edge_dictionary(faces, n_vertices, known_count, dtype):
    want = edge_dictionary(faces)
    t = MT.EdgeTables(torch.from_numpy(faces).to(dtype), n_vertices if known_count else None, with_order=True)
    plain = MT.EdgeTables(torch.from_numpy(faces).to(dtype), n_vertices if known_count else None)      # torch.unique's own sort
    assert plain.order is None
    for field in ("edges", "half_edge_to_edge", "edge_count"):
        assert getattr(plain, field).dtype == torch.int32 and torch.equal(getattr(plain, field), getattr(t, field)), field
    F, E = len(faces), len(want)
    assert (t.edges.dtype, t.half_edge_to_edge.dtype, t.edge_count.dtype, t.order.dtype) == (torch.int32,) * 3 + (torch.int64,)
    assert (tuple(t.edges.shape), tuple(t.half_edge_to_edge.shape), tuple(t.edge_count.shape), tuple(t.order.shape)) == ((E, 2), (3 * F,), (E,), (3 * F,))
    edges = [tuple(e) for e in t.edges.tolist()]
    assert edges == sorted(want)                                        # unique, ascending in (u, v)
    h2e, count, order = t.half_edge_to_edge.tolist(), t.edge_count.tolist(), t.order.tolist()
    for h in range(3 * F):                                              # every half-edge maps to the edge of its two vertices
        a, b = faces[h // 3][h % 3], faces[h // 3][(h % 3 + 1) % 3]
        assert edges[h2e[h]] == (min(a, b), max(a, b))
    assert sum(count) == 3 * F and count == [len(want[e]) for e in edges]
    first = 0
    for e, n in zip(edges, count):                                      # `order`: each edge's half-edges, contiguous and ascending
        assert order[first:first + n] == want[e]
        first += n


@cases
def test_adjacency_and_border_count_agree_with_the_counts(faces, n_vertices):
    want = edge_dictionary(faces)
    pairs = [(h[0] // 3, h[1] // 3) for _, h in sorted(want.items()) if len(h) == 2]        # in the order of their edge, lower face first
    adj = mesh_cleanup.face_adjacency(torch.from_numpy(faces))
    assert adj.dtype == torch.int64 and adj.tolist() == [list(p) for p in pairs]
    assert isosurface.border_edge_count(torch.from_numpy(faces)) == sum(len(h) == 1 for h in want.values())
    counts = MT.EdgeTables(torch.from_numpy(faces), n_vertices).edge_count
    assert len(pairs) == int((counts == 2).sum()) and isosurface.border_edge_count(torch.from_numpy(faces)) == int((counts == 1).sum())


def test_the_tables_of_an_empty_face_array():
    for with_order in (False, True):
        t = MT.EdgeTables(torch.zeros((0, 3), dtype=torch.int64), 5, with_order=with_order)
        assert tuple(t.edges.shape) == (0, 2) and t.half_edge_to_edge.numel() == t.edge_count.numel() == 0
    assert t.order.numel() == 0
    assert isosurface.border_edge_count(torch.zeros((0, 3), dtype=torch.int64)) == 0


@cases
def test_referenced_vertices_and_compact_rows(faces, n_vertices):
    n = n_vertices + 3                                                  # three vertices that no face names, at the end
    used, rank = MT.referenced_vertices(torch.from_numpy(faces), n)
    names = np.unique(faces)
    assert used.dtype == torch.bool and rank.dtype == torch.int64
    assert np.array_equal(np.flatnonzero(used.numpy()), names)
    assert np.array_equal(rank.numpy()[names], np.arange(len(names)))   # kept vertices keep their order
    assert np.array_equal(names[rank.numpy()[faces]], faces)            # and the re-indexed faces name the same vertices
    rows = torch.arange(n * 3, dtype=torch.float64).reshape(n, 3)
    kept = MT.compact_rows(rows, used, len(names))
    assert kept.is_contiguous() and np.array_equal(kept.numpy(), rows.numpy()[used.numpy()])
    short = MT.compact_rows(rows, used, len(names) - 1)                 # rows beyond n_keep are cut off, not written over others
    assert np.array_equal(short.numpy(), rows.numpy()[used.numpy()][:-1])
    assert MT.compact_rows(rows, torch.zeros(n, dtype=torch.bool), 0).shape == (0, 3)


def sparse_icosphere_faces():
    from test_render_gpu import sparse_icosphere            # 2562 used vertices scattered over 3072 rows
    return sparse_icosphere()[1]


@pytest.mark.parametrize("faces,n_vertices", [(sparse_icosphere_faces, 3072), (lambda: RANDOM_FACES, N_RANDOM_VERTICES),
                                              (lambda: np.array([[0, 1, 2], [3, 3, 1], [2, 2, 2], [1, 4, 1]]), 6)],
                         ids=["sparse-3072", "random-7x300", "repeats-in-a-face"])
def test_corners_over_three_are_the_faces_on_a_vertex_in_ascending_order(faces, n_vertices):
    """What am_render_normals sums along: `corners[offsets[v] : offsets[v + 1]] // 3` is the ascending list of the faces on v, one
    entry per occurrence of v in a face; a vertex on no face has an empty list."""
    faces = faces()
    want = [[] for _ in range(n_vertices)]
    for f, tri in enumerate(faces.tolist()):
        for v in tri:
            want[v].append(f)
    t = MT.MeshTopology(torch.from_numpy(faces), n_vertices)
    offsets, corners = t.offsets.tolist(), t.corners.tolist()
    assert offsets[0] == 0 and offsets[-1] == 3 * len(faces)
    for v in range(n_vertices):
        assert [c // 3 for c in corners[offsets[v]:offsets[v + 1]]] == want[v], v
    if n_vertices == 6:
        assert want[2] == [0, 2, 2, 2] and want[1] == [0, 1, 3, 3] and want[5] == []
    if n_vertices == 3072:
        assert sum(len(w) == 0 for w in want) == 3072 - 2562


def test_the_names_the_other_modules_keep():
    assert mesh_prep.MeshTopology is MT.MeshTopology and mesh_decimate.MeshTopology is MT.MeshTopology
    assert mesh_decimate.EdgeTables is MT.EdgeTables
