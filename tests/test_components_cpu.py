"""Connected components (INTEGRATION.md seam S9), the parts that need no GPU: the scipy restatement the device tests compare
against (checked here on hand-made cases), `face_adjacency` against a brute-force edge dictionary, the control flow of
`remove_floaters` over a scipy stand-in for `ops.graph_components`, the `install_mask_refine()` seam against the reference's own
`background_removal` module (skipped where the reference checkout is absent), and the
argument validation of the two `ops` wrappers."""
import ctypes
import inspect
import os
import sys
import types

import numpy as np
import pytest
import torch
from scipy import ndimage
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from actionmesh_amd import _lib, mesh_cleanup, ops
from actionmesh_amd.mask_refine import otsu_threshold

REF = "/root/reference"
HAVE_REF = os.path.isdir(os.path.join(REF, "actionmesh"))
needs_ref = pytest.mark.skipif(not HAVE_REF, reason="reference not present")


# ---- the restatements the device tests import ------------------------------------------------------------------------------------
def canonical_labels(fg: np.ndarray, structure=None) -> np.ndarray:
    """int32 labels of a boolean (H, W) image: 0 on background, 1 + min(y * W + x) over the pixel's component (8-connected unless
    another `structure` is given), from scipy.ndimage.label."""
    lab, n = ndimage.label(fg, structure=np.ones((3, 3), int) if structure is None else structure)
    out = np.zeros(fg.shape, np.int32)
    if n:
        flat = lab.reshape(-1)
        first = np.full(n + 1, fg.size, np.int64)
        np.minimum.at(first, flat, np.arange(fg.size))
        out = np.where(lab > 0, first[lab] + 1, 0).astype(np.int32)
    return out


def refine_restatement(mask: np.ndarray, min_size: int = 200, threshold=None):
    """(out_mask uint8, labels int32, stats int32[4]) of one (H, W) uint8 frame: otsu_threshold (or the fixed threshold),
    scipy.ndimage.label with the full 3 x 3 structure, np.bincount for the sizes, size >= min_size kept."""
    thr = int(otsu_threshold(mask)) if threshold is None else int(threshold)
    fg = mask > thr
    lab, n = ndimage.label(fg, structure=np.ones((3, 3), int))
    sizes = np.bincount(lab.reshape(-1), minlength=n + 1)
    big = sizes >= min_size
    big[0] = False
    out = np.where(big[lab], 255, 0).astype(np.uint8)
    stats = np.array([thr, int(fg.sum()), n, int(big.sum())], np.int32)
    return out, canonical_labels(fg), stats


def graph_restatement(n_nodes: int, edges: np.ndarray):
    """(label, size) int32 of every node: scipy's connected components, canonicalised to the smallest node index."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    g = coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n_nodes, n_nodes))
    n, comp = connected_components(g, directed=False)
    first = np.full(n, n_nodes, np.int64)
    np.minimum.at(first, comp, np.arange(n_nodes))
    return first[comp].astype(np.int32), np.bincount(comp, minlength=n)[comp].astype(np.int32)


def checkerboard(h, w):
    y, x = np.mgrid[:h, :w]
    return np.where((x + y) % 2 == 0, 255, 0).astype(np.uint8)


# ---- the restatement on hand-made cases ------------------------------------------------------------------------------------------
def test_checkerboard_is_one_component_only_through_diagonals():
    m = checkerboard(6, 7)
    out, lab, stats = refine_restatement(m, min_size=1)
    assert stats.tolist() == [0, 21, 1, 1] and np.array_equal(out, m)
    assert set(np.unique(lab)) == {0, 1}                                               # pixel (0, 0) is the smallest: label 1
    four = canonical_labels(m > 0, structure=ndimage.generate_binary_structure(2, 1))
    assert len(np.unique(four[four > 0])) == 21                                        # 4-connected: every pixel on its own


def test_constant_and_empty_images():
    for v in (0, 7, 255):
        assert int(otsu_threshold(np.full((5, 9), v, np.uint8))) == 0
    out, lab, stats = refine_restatement(np.zeros((4, 4), np.uint8), 1)
    assert not out.any() and not lab.any() and stats.tolist() == [0, 0, 0, 0]
    out, lab, stats = refine_restatement(np.full((4, 4), 9, np.uint8), 1)              # constant and above threshold 0: all foreground
    assert (out == 255).all() and (lab == 1).all() and stats.tolist() == [0, 16, 1, 1]


def test_otsu_on_hand_made_histograms():
    two = np.array([[10] * 8 + [200] * 8], np.uint8)
    assert int(otsu_threshold(two)) == 10                                              # the first maximum: every i in 10 .. 199 ties
    assert otsu_threshold(np.stack([two, two])).tolist() == [10, 10] and otsu_threshold(torch.from_numpy(two)).dtype == np.int32
    outlier = np.zeros((4096, 4096), np.uint8)                                         # one pixel in 2^24: q2 < FLT_EPSILON, every bin skipped
    outlier[0, 0] = 255
    assert int(otsu_threshold(outlier)) == 0
    with pytest.raises(TypeError):
        otsu_threshold(np.zeros((4, 4), np.float32))


def test_canonical_labels_and_size_rule():
    m = np.zeros((5, 8), np.uint8)
    m[0, 5:8] = 255            # 3 pixels, first index 5
    m[2:4, 0:2] = 255          # 4 pixels, first index 16
    m[4, 2] = 255              # touches (3, 1) diagonally: same component, 5 pixels
    out, lab, stats = refine_restatement(m, min_size=4)
    assert sorted(np.unique(lab)) == [0, 6, 17] and lab[4, 2] == 17
    assert stats.tolist() == [0, 8, 2, 1] and out[0, 5] == 0 and out[4, 2] == 255      # size 3 < 4 removed, size 5 kept
    assert refine_restatement(m, min_size=3)[2][3] == 2 and refine_restatement(m, min_size=6)[2][3] == 0


def test_graph_restatement():
    lab, size = graph_restatement(6, np.array([[4, 2], [2, 2], [5, 4], [0, 3], [0, 3]]))
    assert lab.tolist() == [0, 1, 2, 0, 2, 2] and size.tolist() == [2, 1, 3, 2, 3, 3]
    lab, size = graph_restatement(3, np.zeros((0, 2), np.int64))
    assert lab.tolist() == [0, 1, 2] and size.tolist() == [1, 1, 1]


# ---- face_adjacency ----------------------------------------------------------------------------------------------------------------
def brute_adjacency(faces: np.ndarray):
    edges = {}
    for f, tri in enumerate(faces):
        for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
            edges.setdefault((min(a, b), max(a, b)), []).append(f)
    return sorted(tuple(sorted(v)) for v in edges.values() if len(v) == 2)


OCTAHEDRON = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
STRIP = np.array([[0, 1, 2], [2, 1, 3], [2, 3, 4], [4, 3, 5]])
FAN = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4], [2, 1, 5]])        # edge 0-1 carries three faces; face 3 hangs on face 0 by edge 1-2


@pytest.mark.parametrize("faces", [OCTAHEDRON, STRIP, FAN], ids=["closed", "open-strip", "three-on-an-edge"])
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_face_adjacency_against_the_edge_dictionary(faces, dtype):
    adj = mesh_cleanup.face_adjacency(torch.from_numpy(faces).to(dtype))
    assert adj.dtype == torch.int64 and adj.dim() == 2 and adj.shape[1] == 2
    assert sorted(tuple(sorted(p)) for p in adj.tolist()) == brute_adjacency(faces)


def test_face_adjacency_cases_by_hand():
    assert len(mesh_cleanup.face_adjacency(torch.from_numpy(OCTAHEDRON))) == 12        # closed: every edge pairs two faces
    assert sorted(map(tuple, mesh_cleanup.face_adjacency(torch.from_numpy(STRIP)).tolist())) == [(0, 1), (1, 2), (2, 3)]
    assert mesh_cleanup.face_adjacency(torch.from_numpy(FAN)).tolist() == [[0, 3]]      # the triple edge pairs nobody
    assert mesh_cleanup.face_adjacency(torch.zeros((0, 3), dtype=torch.int64)).shape == (0, 2)
    with pytest.raises(ValueError):
        mesh_cleanup.face_adjacency(torch.zeros((4, 4), dtype=torch.int64))
    with pytest.raises(TypeError):
        mesh_cleanup.face_adjacency(torch.zeros((4, 3)))


# ---- remove_floaters over a scipy stand-in for the kernel -----------------------------------------------------------------------
@pytest.fixture
def scipy_components(monkeypatch):
    def graph_components(n_nodes, edges, return_size=False):
        assert edges.dtype == torch.int32 and edges.is_contiguous() and edges.dim() == 2
        lab, size = graph_restatement(n_nodes, edges.numpy())
        return (torch.from_numpy(lab), torch.from_numpy(size)) if return_size else torch.from_numpy(lab)
    monkeypatch.setattr(ops, "graph_components", graph_components)


def _two_strips_and_a_floater():
    """strip A (faces 0-3, vertices 0-5), one unreferenced vertex 6, a single triangle (face 4, vertices 7-9), strip B (faces 5-8,
    vertices 10-15); the floater sits between the strips so that re-indexing has something to close up."""
    faces = np.concatenate([STRIP, [[7, 8, 9]], STRIP + 10])
    verts = np.arange(16 * 3, dtype=np.float32).reshape(16, 3)
    return torch.from_numpy(verts), torch.from_numpy(faces)


def test_remove_floaters_one_component_returns_the_same_objects(scipy_components):
    v, f = torch.randn(6, 3), torch.from_numpy(STRIP)
    out = mesh_cleanup.remove_floaters(v, f, threshold=0.5)
    assert out[0] is v and out[1] is f
    v2, f2, vi, fi = mesh_cleanup.remove_floaters(v, f, threshold=0.5, return_index=True)
    assert v2 is v and f2 is f and vi.tolist() == list(range(6)) and fi.tolist() == list(range(4))
    e = torch.zeros((0, 3), dtype=torch.int64)
    assert mesh_cleanup.remove_floaters(v, e)[1] is e


def test_remove_floaters_thresholds(scipy_components):
    v, f = _two_strips_and_a_floater()
    lab, size = mesh_cleanup.face_components(f)
    assert lab.tolist() == [0, 0, 0, 0, 4, 5, 5, 5, 5] and size.tolist() == [4, 4, 4, 4, 1, 4, 4, 4, 4]
    # threshold 0 (the signature's default): min_faces = 0, every component kept - but the unreferenced vertex goes, as in mesh.split
    v0, f0, vi, fi = mesh_cleanup.remove_floaters(v, f, return_index=True)
    assert fi.tolist() == list(range(9)) and vi.tolist() == [i for i in range(16) if i != 6]
    assert torch.equal(v0[f0], v[f])
    # 0.26 * 4 = 1.04 -> min_faces 1: still everything; 0.5 -> 2: the floater goes, the two equal strips stay
    assert mesh_cleanup.remove_floaters(v, f, 0.26)[1].shape[0] == 9
    v1, f1, vi, fi = mesh_cleanup.remove_floaters(v, f, 0.5, return_index=True)
    assert fi.tolist() == [0, 1, 2, 3, 5, 6, 7, 8] and vi.tolist() == list(range(6)) + list(range(10, 16))
    assert f1.dtype == f.dtype and f1.tolist() == np.concatenate([STRIP, STRIP + 6]).tolist()      # exact re-indexing
    assert torch.equal(v1, v[vi]) and torch.equal(v1[f1], v[f[fi]])
    assert mesh_cleanup.remove_floaters(v, f, 1.0)[1].shape[0] == 8                    # both equal components meet max_faces itself
    # above 1: nothing would be kept -> the input, as the reference returns the mesh
    out = mesh_cleanup.remove_floaters(v, f, 1.5)
    assert out[0] is v and out[1] is f


def test_remove_floaters_animated_vertices(scipy_components):
    v, f = _two_strips_and_a_floater()
    anim = torch.stack([v, v + 100.0, v - 3.0])
    va, fa, vi, fi = mesh_cleanup.remove_floaters(anim, f, 0.5, return_index=True)
    assert va.shape == (3, 12, 3) and torch.equal(va, anim[:, vi]) and fa.shape == (8, 3)
    with pytest.raises(ValueError):
        mesh_cleanup.remove_floaters(torch.zeros(16, 2), f)


# ---- the seam --------------------------------------------------------------------------------------------------------------------
@needs_ref
def test_install_mask_refine_swaps_the_references_function(monkeypatch):
    """The reference's own background_removal module, imported with stand-ins for the libraries it needs at import time (cv2, skimage,
    torchvision, transformers are not all present here), and a stand-in `actionmesh.pipeline` for install()."""
    from actionmesh_amd import dropin, mask_refine

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)

        def anything(attr):                     # `from skimage.measure import label`, `mesh: trimesh.Trimesh`, ...: any public name resolves
            if attr.startswith("__"):
                raise AttributeError(attr)
            return type(attr, (), {})
        m.__getattr__ = anything
        monkeypatch.setitem(sys.modules, name, m)
        return m

    for name in ("cv2", "skimage", "skimage.measure", "skimage.morphology", "torchvision", "torchvision.transforms",
                 "torchvision.transforms.functional", "transformers", "trimesh"):
        stub(name)
    for name in [n for n in sys.modules if n == "actionmesh" or n.startswith("actionmesh.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.syspath_prepend(REF)
    import actionmesh.preprocessing.background_removal as B
    P = stub("actionmesh.pipeline", ActionMeshDenoiser=type("ActionMeshDenoiser", (), {}), load_config=lambda name, d: {})
    monkeypatch.setattr(sys.modules["actionmesh"], "pipeline", P, raising=False)
    original = B.refine_mask
    assert original.__module__ == "actionmesh.preprocessing.background_removal"
    try:
        dropin.install()
        assert B.refine_mask is original                                               # install() alone leaves it
        dropin.install_mask_refine()
        dropin.install_mask_refine()                                                   # idempotent
        assert B.refine_mask is mask_refine.refine_mask
        assert inspect.signature(B.refine_mask) == inspect.signature(original)
        dropin.install()                                                               # a fresh install() takes it back
        assert B.refine_mask is original
        dropin.uninstall()
        dropin.install_mask_refine()                                                   # on its own: install() first
        assert dropin.is_installed() and B.refine_mask is mask_refine.refine_mask
        dropin.uninstall()
        assert B.refine_mask is original
    finally:
        dropin.uninstall()


def test_refine_mask_keeps_the_recorded_signature():
    """Where the reference is absent: refine_mask(mask: np.ndarray, min_size: int = 200) -> np.ndarray, as background_removal.py:20."""
    from actionmesh_amd.mask_refine import refine_mask
    sig = inspect.signature(refine_mask)
    assert [(n, p.default) for n, p in sig.parameters.items()] == [("mask", inspect.Parameter.empty), ("min_size", 200)]


def test_cli_flag():
    from actionmesh_amd import cli
    assert cli.split_args([])[0].mask_refine == "off"
    ours, rest = cli.split_args(["--mask-refine", "hip", "--", "--input", "x"])
    assert ours.mask_refine == "hip" and rest == ["--input", "x"]
    with pytest.raises(SystemExit):
        cli.split_args(["--mask-refine", "auto"])


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------------
def test_entry_points_validate_before_launch():
    """Bad arguments are refused on the host, before any launch (no device is touched here)."""
    lib = _lib.lib()
    assert lib.am_mask_refine(None, None) != 0 and b"null" in lib.am_last_error()
    assert lib.am_graph_components(None, None) != 0 and b"null" in lib.am_last_error()
    assert lib.am_mask_refine_workspace_bytes(2, 33, 47) >= 2 * 4 * 2 * 33 * 47 + 2 * 1024 + 8
    assert lib.am_mask_refine_workspace_bytes(0, 4, 4) == 0 and lib.am_graph_components_workspace_bytes(0, 0) == 0
    a = _lib.AmMaskRefineArgs()
    a.mask = a.out_mask = 4096
    a.n_frames, a.height, a.width, a.min_size, a.threshold = 1, 65536, 32768, 1, -1
    assert lib.am_mask_refine(ctypes.byref(a), None) != 0 and b"32-bit" in lib.am_last_error()
    a.height, a.width, a.min_size = 8, 8, -1
    assert lib.am_mask_refine(ctypes.byref(a), None) != 0 and b"min_size" in lib.am_last_error()
    a.min_size, a.threshold = 0, 256
    assert lib.am_mask_refine(ctypes.byref(a), None) != 0 and b"threshold" in lib.am_last_error()
    a.threshold = -1
    assert lib.am_mask_refine(ctypes.byref(a), None) != 0 and b"workspace" in lib.am_last_error()
    g = _lib.AmGraphArgs()
    g.out_label = g.out_flag = 4096
    assert lib.am_graph_components(ctypes.byref(g), None) != 0 and b"nodes" in lib.am_last_error()
    g.n_nodes, g.n_edges = 4, 2
    assert lib.am_graph_components(ctypes.byref(g), None) != 0 and b"null" in lib.am_last_error()
    g.edges = 4096
    assert lib.am_graph_components(ctypes.byref(g), None) != 0 and b"workspace" in lib.am_last_error()


def test_ops_argument_validation():
    """dtype, rank, contiguity, min_size < 0, threshold outside -1 .. 255 - and, last, the device: there is no CPU path."""
    ok = torch.zeros((2, 8, 8), dtype=torch.uint8)
    with pytest.raises(TypeError):
        ops.mask_refine(ok.float())
    with pytest.raises(TypeError):
        ops.mask_refine(ok.numpy())
    with pytest.raises(ValueError):
        ops.mask_refine(ok[0])
    with pytest.raises(ValueError):
        ops.mask_refine(ok[:, :, :0])
    with pytest.raises(ValueError):
        ops.mask_refine(ok.transpose(1, 2)[:, :, ::2])
    with pytest.raises(ValueError):
        ops.mask_refine(ok, min_size=-1)
    for thr in (-2, 256):
        with pytest.raises(ValueError):
            ops.mask_refine(ok, threshold=thr)
    with pytest.raises(RuntimeError):
        ops.mask_refine(ok)
    e = torch.zeros((3, 2), dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.graph_components(4, e.long())
    with pytest.raises(ValueError):
        ops.graph_components(4, e.reshape(-1))
    with pytest.raises(ValueError):
        ops.graph_components(4, torch.zeros((3, 4), dtype=torch.int32)[:, ::2])
    with pytest.raises(ValueError):
        ops.graph_components(0, e)
    with pytest.raises(RuntimeError):
        ops.graph_components(4, e)
    from actionmesh_amd.mask_refine import refine_masks
    with pytest.raises(TypeError):
        refine_masks(np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError):
        refine_masks(np.zeros((4,), np.uint8))
