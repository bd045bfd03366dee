"""am_render_normals on the device against the integer reference of tests/_raster_exact.py on EVERY sub-pixel of every image - no
stability mask - and, on three perspective scenes of tests/test_render_gpu.py, bit for bit against the fp32 restatement of
tests/_raster_emulation.py.

On the exact scenes pix_to_face and the mask must equal the reference; the barycentrics are exactly -1 where nothing covers and
within gamma_7 = 7u / (1 - 7u), u = 2^-24, of the exact rational E_i / A elsewhere (the count is in _raster_exact.compare); normals
are exactly (0.5, 0.5, 1) where the view normal is +z or 0, within 6.5u of fp64 on a tilted patch, and the bytes are equal at every
pixel (every one is exactly computable or at least 1e-3 from a byte boundary: _raster_exact.image asserts it).

Every test runs am_render_normals of both library builds (the bfloat16 one, which render.py calls, and the float16 one: the same
source, built a second time).

Records, not thresholds (MI355X, both builds alike): largest barycentric err / bound 0.2857 on every exact scene (2 of the 7
counted roundings), largest tilted-normal err / bound 0.0613; on the general scenes no face index and no barycentric bit differs
on 49152 + 16384 + 16384 sub-pixels."""
import numpy as np
import pytest
import torch

import _raster_emulation as E
import _raster_exact as X
from actionmesh_amd import render as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(params=["bf16", "f16"], autouse=True)
def build(request, monkeypatch):
    """The entry points without 16-bit code are looked up with no key, which means the bfloat16 build: give them this one."""
    from actionmesh_amd import ops
    entry = ops._entry
    monkeypatch.setattr(ops, "_entry", lambda key, name: entry(request.param if key is None else key, name))
    return request.param


def render(verts, faces, cams, S):
    out = R.HipRenderer(S).render_normals(torch.as_tensor(verts, dtype=torch.float32).to(DEV), torch.as_tensor(faces), cams,
                                          return_fragments=True, return_float=True)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in out.items()}


def check_scene(name):
    scene, refs = X.reference(name)
    W = 2 * scene["S"]
    got = render(X.float_verts(scene), scene["faces"], [X.torch_camera(c, W) for c in scene["cams"]], scene["S"])
    assert got["pix_to_face"].shape == (len(scene["verts"]), len(scene["cams"]), W, W)
    worst = [X.compare({k: v[t, c] for k, v in got.items()}, ref, f"{name} frame {t} camera {c}") for (t, c), ref in refs.items()]
    print(f"{name}: {len(refs)} images of {W} x {W} sub-pixels, every one compared; largest barycentric err / bound "
          f"{max(w[0] for w in worst):.4f}, largest tilted-normal err / bound {max(w[1] for w in worst):.4f}")
    return got, refs


def test_faces_straddling_the_camera_plane_decide_the_closed_box():
    """Two vertices behind the camera: the cone of positive barycentrics is covered up to and ON the edges of the box of the
    projected vertices, which lie on centres, and not beyond; one vertex behind: nothing is covered (negative depth).  Face index,
    mask, alpha and the -1 of uncovered barycentrics on every sub-pixel; no normal is stated for these faces."""
    check_scene("straddle")


def test_tiling_edges_vertices_and_both_orientations():
    """Centres on shared edges and on vertices belong to neither face; zero-area triangles and slivers between centres cover
    nothing; patches that look away show (0.5, 0.5, 1) exactly, tilted patches that look at the camera show +x, -x and +y, and the
    normal 0 of an uncovered (2i, 2j) sub-pixel shows (0.5, 0.5, 1) under a partial mask: a normal read from another sub-pixel
    changes a colour."""
    got, refs = check_scene("tiling")
    ref = refs[0, 0]
    shown = ref["mask_q"] > 0
    assert len({tuple(np.round(v, 3)) for v in got["normal"][0, 0][shown].tolist()}) == 4, "+z, +x, -x and +y"
    assert (shown & (ref["face"][::2, ::2] < 0)).any()


def test_box_edges_image_border_and_a_face_behind_the_camera():
    """Box edges on centres, the sub-pixel rows and columns 0 and W - 1, faces partly and wholly outside on the four sides and over
    the corners, one frame-filling face behind the camera."""
    check_scene("border")


def test_depth_planes_in_every_index_order_and_ties_to_the_lowest_index():
    """Planes 1, 2, 4 in the six index orders; duplicates at the highest indices lose to their first copy, on the same vertex rows
    and on rows of their own; a queued face between a nearer and a farther face the raster thread tests itself."""
    check_scene("depth")


def test_path_switch_at_small_box_and_thin_boxes():
    """Loop boxes 5 x 5 .. 11 x 11 (SMALL_BOX = 64: up to 8 x 8 the raster thread, from 9 x 9 the queue), each with the corner on a
    centre and between centres, and 12 x 5 (thread), 13 x 5, 16 x 5, 20 x 5 (queue) wide and tall: a row / column swap in the split
    of raster_big_kernel leaves the box.  tests/test_raster_exact_cpu.py asserts these sizes from the loop bounds."""
    check_scene("paths")


def test_queue_of_more_than_big_blocks_faces_over_a_batch_of_images():
    """1101 faces, every one queued, in 2 frames x 3 cameras: 5196 queue entries for 1024 blocks, so the stride loop runs up to six
    times and every entry's img * F + f code is decoded with F = 1101.  Each image against its own reference."""
    check_scene("queue")


@pytest.mark.parametrize("name", ["jittered_icosphere", "straddlers", "frame_filling_quad"])
def test_general_scene_is_the_fp32_restatement_bit_for_bit(name):
    """pix_to_face, bary (bitwise) and mask on every sub-pixel at S = 64, the unstable ones included: only IEEE add, multiply,
    divide and max enter them.  (Normals and bytes of these scenes involve sqrtf and stay with the fp64 test.)"""
    V, F, cams = E.general_scenes()[name]
    got = render(np.asarray(V, dtype=np.float64).astype(np.float32)[None], F, cams, 64)
    want = E.render_batch(V, F, cams, 64, normals=False)
    face_diff = got["pix_to_face"] != want["pix_to_face"]
    bary_diff = (got["bary"].view(np.uint32) != want["bary"].view(np.uint32)).any(-1)
    print(f"{name}: {face_diff.size} sub-pixels, {int((want['pix_to_face'] >= 0).sum())} covered; face differs on "
          f"{int(face_diff.sum())}, barycentric bits on {int(bary_diff.sum())}")
    assert not face_diff.any(), np.argwhere(face_diff)[:5]
    assert not bary_diff.any(), np.argwhere(bary_diff)[:5]
    assert np.array_equal(got["mask"], want["mask"])
