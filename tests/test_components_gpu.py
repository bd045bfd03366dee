"""Connected components on the device (csrc/am_components.hip through ops.mask_refine / ops.graph_components, mask_refine.py and
mesh_cleanup.py).  The contract of include/actionmesh_amd.h has no tolerance: out_mask, out_labels and out_stats are compared BIT FOR
BIT with the scipy restatement of tests/test_components_cpu.py, the threshold with `otsu_threshold`, graph labels and sizes with
scipy's connected components canonicalised to the smallest index - no case exempted."""
import numpy as np
import pytest
import torch

from actionmesh_amd import mask_refine as MR
from actionmesh_amd import mesh_cleanup, ops
from test_components_cpu import (FAN, OCTAHEDRON, checkerboard, graph_restatement, refine_restatement)   # tests/ is on sys.path

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _check(frames, min_size, threshold=None):
    """One call over all `frames` (a list of equal-sized (H, W) uint8 arrays) against the restatement of every frame; returns the
    device results as numpy (mask, labels, stats)."""
    batch = np.stack(frames)
    out, lab, stats = MR.refine_masks(torch.from_numpy(batch).to(DEV), min_size=min_size, threshold=threshold, return_labels=True,
                                      return_stats=True)
    assert (out.dtype, lab.dtype, stats.dtype) == (torch.uint8, torch.int32, torch.int32)
    assert out.shape == lab.shape == batch.shape and stats.shape == (len(frames), 4) and out.is_cuda
    out, lab, stats = out.cpu().numpy(), lab.cpu().numpy(), stats.cpu().numpy()
    for t, frame in enumerate(frames):
        want_out, want_lab, want_stats = refine_restatement(frame, min_size, threshold)
        assert stats[t].tolist() == want_stats.tolist(), f"frame {t}: stats {stats[t].tolist()} != {want_stats.tolist()}"
        bad = np.flatnonzero(lab[t].reshape(-1) != want_lab.reshape(-1))
        assert bad.size == 0, f"frame {t}: {bad.size} labels differ, first at pixel {bad[0]}: {lab[t].reshape(-1)[bad[0]]} != {want_lab.reshape(-1)[bad[0]]}"
        assert np.array_equal(out[t], want_out), f"frame {t}: out_mask differs in {int((out[t] != want_out).sum())} pixels"
    return out, lab, stats


def _u8(a):
    return np.where(a, 255, 0).astype(np.uint8)


def test_smallest_shapes():
    """1 x 1 foreground and background, 1 x W, H x 1, the 2 x 2 diagonal (joined only through the corner)."""
    _, lab, stats = _check([np.full((1, 1), 255, np.uint8)], 1)
    assert lab.tolist() == [[[1]]] and stats.tolist() == [[0, 1, 1, 1]]
    _, lab, stats = _check([np.zeros((1, 1), np.uint8)], 1)
    assert lab.tolist() == [[[0]]] and stats.tolist() == [[0, 0, 0, 0]]
    row = _u8(np.array([[1, 1, 0, 1, 0, 0, 1, 1, 1] * 9]))             # 1 x 81: more than two tiles wide
    _, lab, _ = _check([row], 2)
    assert lab[0, 0, :4].tolist() == [1, 1, 0, 4]
    _check([np.ascontiguousarray(row.T)], 2)                            # 81 x 1
    _, lab, stats = _check([_u8(np.eye(2)), _u8(np.eye(2)[::-1])], 2)
    assert lab[0].tolist() == [[1, 0], [0, 1]] and lab[1].tolist() == [[0, 2], [2, 0]] and stats[:, 2].tolist() == [1, 1]


def spiral(h, w):
    """A one-pixel-wide rectangular spiral from the top-left corner inwards, arms one blank pixel apart: ONE component whose
    pixels are joined along a path about h * w / 2 long."""
    m = np.zeros((h, w), bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    inside = lambda a, b: 0 <= a < h and 0 <= b < w
    while True:
        for _ in range(2):
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if inside(ny, nx) and not m[ny, nx] and not (inside(ay, ax) and m[ay, ax]):
                y, x = ny, nx
                m[y, x] = True
                break
            dy, dx = dx, -dy
        else:
            return m


def patterns(h, w):
    diag = np.zeros((h, w), bool)
    for i in range(min(h, w)):
        diag[i, i] = diag[i, w - 1 - i] = True
    frame = np.zeros((h, w), bool)
    frame[0, :] = frame[-1, :] = frame[:, 0] = frame[:, -1] = True
    frame[h // 2, w // 2] = True                                        # and one pixel on its own
    comb = np.zeros((h, w), bool)
    comb[:, ::2] = True                                                 # teeth from the top, joined only by the last row
    comb[-1, :] = True
    teeth = np.zeros((h, w), bool)
    teeth[:, ::2] = True                                                # the same without the spine: w / 2 components
    return [checkerboard(h, w), _u8(diag), _u8(frame), _u8(comb), _u8(teeth), _u8(spiral(h, w))]


@pytest.mark.parametrize("h,w", [(33, 47), (257, 300)])
def test_tile_borders(h, w):
    """Sizes that are no multiple of the 32 x 32 tile and span at least two tiles each way.  The checkerboard joins only through
    diagonals (tile corners included); the spiral is the long-path case of the flatten step."""
    _, lab, stats = _check(patterns(h, w), 2)
    assert stats[0, 2] == 1 and stats[3, 2] == 1 and stats[5, 2] == 1 and stats[4, 2] == (w + 1) // 2
    assert stats[2, 2:].tolist() == [2, 1]                              # the ring stays, the single pixel goes
    assert set(np.unique(lab[5])) == {0, 1}


def test_size_boundary():
    """Three isolated rectangles of 199, 200 and 201 pixels: size >= min_size stays."""
    m = np.zeros((70, 230), bool)
    m[1:2, 3:202] = True            # 1 x 199
    m[10:20, 40:60] = True          # 10 x 20
    m[30:33, 100:167] = True        # 3 x 67
    m = _u8(m)
    out, lab, stats = _check([m], 200)
    assert stats[0].tolist() == [0, 600, 3, 2] and out[0, 1, 3] == 0 and out[0, 10, 40] == 255 and out[0, 30, 100] == 255
    for min_size, kept in ((0, 3), (1, 3), (199, 3), (201, 1), (202, 0), (70 * 230 + 1, 0)):
        assert _check([m], min_size)[2][0, 3] == kept


def test_many_components():
    """rng.random((257, 300)) < 0.41: with the numpy and scipy of the machine this was written on the restatement finds 1143
    components, the largest of 14346 pixels, 14 of at least 200, none of exactly 199 or 200 (the figures are not asserted: they
    are the restatement's, which is what the device is held to)."""
    fg = np.random.default_rng(0).random((257, 300)) < 0.41
    m = _u8(fg)
    _, lab, stats = _check([m], 200)
    sizes = np.sort(np.bincount(lab[0][lab[0] > 0]))[::-1]
    assert len(sizes) > 12 and stats[0, 2] == np.count_nonzero(sizes)
    twelfth = int(sizes[11])
    _, _, stats = _check([m], twelfth)
    assert stats[0, 3] == int((sizes >= twelfth).sum()) >= 12
    _check([m], twelfth + 1)


def test_otsu_threshold_exact():
    """The threshold in out_stats equals otsu_threshold exactly: random images, two-level images, a symmetric two-peak histogram
    (the first maximum wins), a constant image; a fixed threshold skips Otsu."""
    rng = np.random.default_rng(1)
    frames = [rng.integers(0, 256, (16, 16), dtype=np.uint8) for _ in range(32)]
    frames += [np.clip(rng.normal(rng.integers(40, 200), rng.integers(5, 60), (16, 16)), 0, 255).astype(np.uint8) for _ in range(32)]
    frames += [np.where(rng.random((16, 16)) < p, hi, lo).astype(np.uint8)
               for lo, hi, p in ((0, 255, 0.5), (0, 1, 0.3), (254, 255, 0.9), (10, 200, 0.01), (100, 101, 0.5), (0, 128, 0.7))]
    two_peak = np.zeros((16, 16), np.uint8)
    two_peak[:, :4], two_peak[:, 4:8], two_peak[:, 8:12], two_peak[:, 12:] = 50, 60, 190, 200
    frames += [two_peak, np.full((16, 16), 77, np.uint8), np.zeros((16, 16), np.uint8), np.full((16, 16), 255, np.uint8)]
    _, _, stats = _check(frames, 1)
    want = MR.otsu_threshold(np.stack(frames))
    assert stats[:, 0].tolist() == want.tolist()
    assert len(set(want.tolist())) > 30 and want[-3:].tolist() == [0, 0, 0]
    assert stats[-4, 0] == int(MR.otsu_threshold(two_peak)) and 60 <= stats[-4, 0] < 190
    _, _, stats = _check(frames[:8], 1, threshold=127)
    assert stats[:, 0].tolist() == [127] * 8
    _check(frames[:2], 3, threshold=0)
    _check(frames[:2], 3, threshold=255)                                # nothing is above 255


def test_otsu_flt_epsilon_skip():
    """One outlier pixel in 2900 x 2900: its class holds less than FLT_EPSILON of the mass, every bin is skipped, the threshold is 0
    - and the one pixel is a component of its own."""
    m = np.zeros((2900, 2900), np.uint8)
    m[1234, 567] = 255
    _, lab, stats = _check([m], 1)
    assert stats[0].tolist() == [0, 1, 1, 1] and lab[0, 1234, 567] == 1 + 1234 * 2900 + 567


CC_HIST_BLOCK_PIXELS, CC_HIST_MAX_BLOCKS = 256 * 16, 64      # csrc/am_components.hip: CC_THREADS * CC_HIST_CHUNK, CC_HIST_MAX_BLOCKS


def two_trip_frame():
    """601 x 499 = 299 899 pixels: uniform noise in the 262 144 pixels the first trip of cc_hist_kernel's loop reads, a two-level
    distribution in the rest, so the Otsu threshold depends on the second trip; the last chunk holds 11 pixels."""
    h, w = 601, 499
    first_trip = CC_HIST_MAX_BLOCKS * CC_HIST_BLOCK_PIXELS
    # mirrors the launch of cc_hist_kernel in am_mask_refine: min(ceil(hw / 4096), 64) blocks striding by blocks * 4096 pixels
    assert -(-h * w // CC_HIST_BLOCK_PIXELS) > CC_HIST_MAX_BLOCKS and first_trip == 262_144 < h * w < 2 * first_trip
    assert (h * w) % 16 == 11
    rng = np.random.default_rng(0)
    f = np.empty(h * w, np.uint8)
    f[:first_trip] = rng.integers(0, 256, first_trip)
    f[first_trip:] = np.where(rng.random(h * w - first_trip) < 0.7, 235, 180)
    whole, head = int(MR.otsu_threshold(f.reshape(h, w))), int(MR.otsu_threshold(f[:first_trip].reshape(512, 512)))
    assert whole != head, (whole, head)                     # a histogram without the second trip gives another threshold
    return f.reshape(h, w)


def test_histogram_second_trip():
    """more than 64 blocks x 4096 pixels a frame: the grid-stride loop of cc_hist_kernel runs a second, ragged trip - alone and as
    frame 1 of a batch of two; threshold, labels, mask and stats bit for bit"""
    frame = two_trip_frame()
    _, _, stats = _check([frame], 200)
    assert stats[0, 0] == int(MR.otsu_threshold(frame))
    _, _, stats2 = _check([soft_blob(601, 499, 5), frame], 200)
    assert stats2[1].tolist() == stats[0].tolist()


def soft_blob(h, w, seed):
    """A soft disc (a sigmoid of the distance to a jittered centre) plus Gaussian noise, uint8: what a matting network's mask looks
    like to the labelling - one large component, a few thousand specks."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:h, :w]
    cy, cx = h * (0.5 + 0.1 * rng.standard_normal()), w * (0.5 + 0.1 * rng.standard_normal())
    r = np.hypot((y - cy) / h, (x - cx) / w)
    soft = 255.0 / (1.0 + np.exp((r - 0.27) * 40.0))
    return np.clip(soft + 60.0 * rng.standard_normal((h, w)), 0, 255).astype(np.uint8)


def test_product_shape_batch_and_repeat():
    """512 x 512 soft blobs plus noise (frame 0: threshold 116, 5669 components, 59328 pixels kept by the restatement where this was
    written).  Three different frames in one call equal three single-frame calls, and a second run of the same call equals the
    first, bit for bit."""
    frames = [soft_blob(512, 512, s) for s in range(3)]
    out, lab, stats = _check(frames, 200)
    assert stats[0, 0] > 0 and stats[0, 2] > 1000 and stats[0, 3] >= 1
    dev = torch.from_numpy(np.stack(frames)).to(DEV)
    again = MR.refine_masks(dev, return_labels=True, return_stats=True)
    for got, first in zip(again, (out, lab, stats)):
        assert np.array_equal(got.cpu().numpy(), first)
    for t in range(3):
        single = MR.refine_masks(dev[t], return_labels=True, return_stats=True)
        for got, first in zip(single, (out, lab, stats)):
            assert got.shape == first[t].shape and np.array_equal(got.cpu().numpy(), first[t])


def test_refine_mask_numpy_in_numpy_out():
    m = soft_blob(200, 300, 7)
    got = MR.refine_mask(m, min_size=50)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == m.shape and set(np.unique(got)) == {0, 255}
    assert np.array_equal(got, refine_restatement(m, 50)[0])
    assert np.array_equal(MR.refine_mask(m), refine_restatement(m, 200)[0])
    host = MR.refine_masks(m)                                           # a host array in, a device tensor out
    assert host.is_cuda and np.array_equal(host.cpu().numpy(), refine_restatement(m, 200)[0])


# ---- graphs ------------------------------------------------------------------------------------------------------------------------
def _check_graph(n, edges):
    e = torch.from_numpy(np.asarray(edges, np.int32).reshape(-1, 2)).to(DEV)
    lab, size = ops.graph_components(n, e, return_size=True)
    assert lab.dtype == size.dtype == torch.int32 and lab.shape == size.shape == (n,)
    want_lab, want_size = graph_restatement(n, edges)
    assert np.array_equal(lab.cpu().numpy(), want_lab) and np.array_equal(size.cpu().numpy(), want_size)
    assert torch.equal(ops.graph_components(n, e), lab)
    return want_lab


def test_graph_components_against_scipy():
    rng = np.random.default_rng(3)
    lab = _check_graph(5000, rng.integers(0, 5000, (4000, 2)))
    assert len(np.unique(lab)) > 1000
    e = rng.integers(0, 300, (200, 2))
    _check_graph(300, np.concatenate([e, e[::-1], e[:, ::-1], np.stack([np.arange(300), np.arange(300)], 1)]))   # duplicates, self-loops
    _check_graph(7, np.zeros((0, 2), np.int32))
    _check_graph(1, np.zeros((0, 2), np.int32))
    path = np.stack([np.arange(4095), np.arange(1, 4096)], 1)
    lab = _check_graph(4096, path[rng.permutation(4095)])
    assert not lab.any()
    _check_graph(4096, path[::-1, ::-1].copy())
    star = np.stack([np.full(999, 999), np.arange(999)], 1)                 # the hub is the LARGEST index
    assert not _check_graph(1000, star).any()


@pytest.mark.parametrize("bad", [[5, 0], [0, -1], [2 ** 31 - 1, 1]])
def test_graph_components_out_of_range_raises(bad):
    e = torch.tensor([[0, 1], bad, [3, 4]], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="outside"):
        ops.graph_components(5, e)


# ---- remove_floaters ---------------------------------------------------------------------------------------------------------------
def subdivide(verts, faces):
    """Every triangle into four (edge midpoints, shared between neighbours)."""
    verts, mid, out = list(map(tuple, verts)), {}, []

    def m(a, b):
        key = (min(a, b), max(a, b))
        if key not in mid:
            mid[key] = len(verts)
            verts.append(tuple((np.array(verts[a]) + np.array(verts[b])) / 2))
        return mid[key]
    for a, b, c in faces:
        ab, bc, ca = m(a, b), m(b, c), m(c, a)
        out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
    return np.array(verts, np.float32), np.array(out)


def floater_scene():
    """Two octahedra subdivided three times (512 faces, 258 vertices each) with a tetrahedron (4 faces) between them in the arrays."""
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    f = OCTAHEDRON
    for _ in range(3):
        v, f = subdivide(v, f)
    tv = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32) * 0.1 + 5
    tf = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])
    verts = np.concatenate([v, tv, v + 10])
    faces = np.concatenate([f, tf + len(v), f + len(v) + 4])
    return verts, faces, len(v), len(f)


def test_remove_floaters_on_the_device():
    verts, faces, nv, nf = floater_scene()
    assert (nv, nf) == (258, 512)
    v, f = torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV)
    lab, size = mesh_cleanup.face_components(f)
    want_lab, want_size = graph_restatement(len(faces), mesh_cleanup.face_adjacency(torch.from_numpy(faces)).numpy())
    assert np.array_equal(lab.cpu().numpy(), want_lab) and np.array_equal(size.cpu().numpy(), want_size)
    assert sorted(set(want_lab.tolist())) == [0, nf, nf + 4]
    all_v, all_f = list(range(len(verts))), list(range(len(faces)))
    big_v = [i for i in all_v if not nv <= i < nv + 4]
    big_f = [i for i in all_f if not nf <= i < nf + 4]
    for threshold, keep_v, keep_f in ((0.0, all_v, all_f), (0.02, big_v, big_f), (0.5, big_v, big_f)):   # int(512 * 0.02) = 10 > 4
        v2, f2, vi, fi = mesh_cleanup.remove_floaters(v, f, threshold, return_index=True)
        assert vi.tolist() == keep_v and fi.tolist() == keep_f and v2.is_cuda and f2.dtype == f.dtype
        assert torch.equal(v2, v[vi]) and torch.equal(v2[f2], v[f[fi]])
    anim = torch.stack([v, v * 2.0])
    va, fa = mesh_cleanup.remove_floaters(anim, f, 0.02)
    assert va.shape == (2, 2 * nv, 3) and torch.equal(va, anim[:, torch.tensor(big_v, device=DEV)]) and fa.shape == (2 * nf, 3)
    out = mesh_cleanup.remove_floaters(v[:nv], f[:nf], 0.5)                   # one component: the same objects
    assert out[1].data_ptr() == f[:nf].data_ptr() and out[1].shape == (nf, 3)


def test_remove_floaters_fan_with_three_faces_on_one_edge():
    """The edge 0-1 carries three faces and joins nobody: components {0, 3}, {1}, {2}."""
    f = torch.from_numpy(FAN).to(DEV)
    v = torch.randn(6, 3, device=DEV)
    lab, size = mesh_cleanup.face_components(f)
    assert lab.tolist() == [0, 1, 2, 0] and size.tolist() == [2, 1, 1, 2]
    _, _, vi, fi = mesh_cleanup.remove_floaters(v, f, 0.5, return_index=True)         # int(2 * 0.5) = 1: everything stays
    assert fi.tolist() == [0, 1, 2, 3] and vi.tolist() == [0, 1, 2, 3, 4, 5]
    v2, f2, vi, fi = mesh_cleanup.remove_floaters(v, f, 1.0, return_index=True)       # 2: the two single faces go
    assert fi.tolist() == [0, 3] and vi.tolist() == [0, 1, 2, 5] and f2.tolist() == [[0, 1, 2], [2, 1, 3]]
