"""The exact-scene yardstick of tests/test_raster_exact_gpu.py, tested without a GPU: the scenes keep their premises, an fp32 NumPy
restatement of the renderer (tests/_raster_emulation.py) agrees with the integer reference on every sub-pixel and stays inside the
counted bounds, the path-switch scene has the loop boxes its docstring says, and planted faults are rejected by the new comparison.
For every fault the stable-only criterion of tests/test_render_gpu.py (check_against_restatement) is applied to that file's own
scenes and the verdict printed.

Recorded with the emulation: largest barycentric err / bound 0.2857 (2 of the 7 counted roundings), largest tilted-normal
err / bound 0.0613.

The old criterion's verdicts (S = 64): `>=` for `>`, the open box and the tie to the highest index are accepted on all three scenes
(jittered level-2 icosphere under three cameras, the camera-plane straddlers, the frame-filling quad).  The transposed big-face
split is accepted on the two scenes whose queued boxes are square (the quad's and the straddlers' box is the whole image) and
rejected on the icosphere, whose queued boxes are not; a big-face loop without its stride is accepted on all three (at most 960
queue entries); the normal of the wrong sub-pixel is rejected on the icosphere and accepted on the two flat scenes."""
import numpy as np
import pytest

import _raster_emulation as E
import _raster_exact as X

NAMES = list(X.SCENES)


def emulate(name, fault=None):
    scene, refs = X.reference(name)
    V, W = X.float_verts(scene), 2 * scene["S"]
    cams = [X.torch_camera(c, W) for c in scene["cams"]]
    per_image = int(E.queued(E.project(V[0], cams[0]), scene["faces"], W).sum())
    out = {}
    for n, (t, c) in enumerate(refs):
        out[t, c] = E.render(V[t], scene["faces"], cams[c], scene["S"], fault, queue_base=n * per_image)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_scenes_keep_their_conditions(name):
    scene, refs = X.reference(name)
    facts = X.conditions(scene)
    print(f"{name}: S {scene['S']}, {scene['verts'].shape[0]} frames x {len(scene['cams'])} cameras, {len(scene['faces'])} faces: {facts}")
    ref = refs[0, 0]
    if name == "straddle":
        # the cone of positive barycentrics reaches centres ON the box's edges (covered), goes on outside it (not covered), and the
        # face with one vertex behind the camera covers nothing: its depth is negative in the whole cone
        assert facts["cone_on_box_edge"] > 8 and facts["cone_outside_box"] > 100 and facts["depth_rejected"] > 8
        assert ref["strict"].tolist()[2] == 0 and min(ref["strict"].tolist()[:2]) > 20
    if name == "tiling":
        # centres on shared edges and vertices; the five degenerate faces (two zero areas, three slivers) cover nothing
        assert facts["on_edge"] > 50 and facts["zero_area"] == 29 and (ref["strict"][-5:] == 0).all() and ref["strict"][-1] == 0
        assert facts["tilted"] > 10 and facts["uncovered_shown"] > 0
        # the tilted patches show +x, -x and +y; with the (0.5, 0.5, 1) of a patch that looks away and of n = 0: four normals
        assert len({tuple(np.round(v, 3)) for v in ref["normal"][ref["mask_q"] > 0].tolist()}) == 4
        assert ((ref["kind"] == 0) & (ref["face"][::2, ::2] >= 0)).sum() >= 4
    if name == "border":
        assert facts["behind"] == 1 and ref["face"][0].max() >= 0 and ref["face"][-1].max() >= 0
        assert ref["face"][:, 0].max() >= 0 and ref["face"][:, -1].max() >= 0, "the sub-pixel rows and columns 0 and W - 1 are reached"
        assert (ref["strict"] == 0).sum() >= 8, "faces wholly outside and faces whose edge lies on the border cover nothing"
    if name == "depth":
        assert facts["ties"] > 0 and ref["face"].max() < len(scene["faces"]) - 2, "the duplicates at the high indices never show"
        assert (ref["face"] == 0).sum() > 10
    if name == "queue":
        assert len(scene["faces"]) == 1101 and len(refs) == 6


@pytest.mark.parametrize("name", NAMES)
def test_emulation_agrees_with_the_integer_reference(name):
    scene, refs = X.reference(name)
    got = emulate(name)
    worst = [X.compare(got[k], refs[k], f"{name} {k}") for k in refs]
    print(f"{name}: largest barycentric err / bound {max(w[0] for w in worst):.4f}, tilted normal {max(w[1] for w in worst):.4f}")


def test_path_switch_scene_takes_the_paths_it_says():
    """Loop boxes from the emulation's pix_range: the family is 5 x 5 .. 11 x 11 twice (corner on a centre, corner between
    centres), queued from 9 x 9 on; the thin boxes are queued wide (more columns than rows) and tall, and one of each is not."""
    scene, _ = X.reference("paths")
    W = 2 * scene["S"]
    P = E.project(X.float_verts(scene)[0], X.torch_camera(scene["cams"][0], W))
    boxes = []
    for tri in scene["faces"]:
        s = E.face_setup(P, tri, W)
        boxes.append((s[6] - s[5] + 1, s[4] - s[3] + 1))          # columns, rows
    print("loop boxes (columns x rows):", boxes)
    assert boxes[:14] == [(n, n) for n in range(5, 12) for _ in (0, 1)]
    q = E.queued(P, scene["faces"], W)
    assert q[:14].tolist() == [n * n > 64 for n in range(5, 12) for _ in (0, 1)]
    thin = [(b, bool(k)) for b, k in zip(boxes[14:], q[14:])]
    assert any(k and b[0] > 2 * b[1] for b, k in thin) and any(k and b[1] > 2 * b[0] for b, k in thin)
    assert any(not k and b[0] > 2 * b[1] for b, k in thin) and any(not k and b[1] > 2 * b[0] for b, k in thin)
    scene, _ = X.reference("queue")
    W = 2 * scene["S"]
    counts = [int(E.queued(E.project(X.float_verts(scene)[t], X.torch_camera(scene["cams"][c], W)), scene["faces"], W).sum())
              for t in range(2) for c in range(3)]
    print("queued faces per image of the queue scene:", counts)
    # every face is queued under the identity camera; the focal-2 camera pushes some outside the image, which queues nothing
    assert counts[0] == 1101 > E.BIG_BLOCKS and min(counts) > 0 and sum(counts) > 4 * E.BIG_BLOCKS


REJECTED_ON = {"ge": "tiling", "open_box": "straddle", "tie_high": "depth", "transposed_split": "paths", "one_stride": "queue",
               "normal_of_last_subpixel": "tiling"}
# the old criterion on the old file's scenes: True = accepted
OLD_VERDICT = {"ge": (True, True, True), "open_box": (True, True, True), "tie_high": (True, True, True),
               "transposed_split": (False, True, True), "one_stride": (True, True, True),
               "normal_of_last_subpixel": (False, True, True)}


@pytest.mark.parametrize("fault", E.FAULTS)
def test_planted_fault_is_rejected_here_and_what_the_old_criterion_says(fault):
    import test_render_gpu as TR
    name = REJECTED_ON[fault]
    _, refs = X.reference(name)
    got = emulate(name, fault)
    with pytest.raises(AssertionError) as caught:
        for k in refs:
            X.compare(got[k], refs[k], f"{name} {k}")
    print(f"{fault}: rejected on '{name}': {str(caught.value)[:160]}")
    verdicts = []
    for scene, (V, F, cams) in E.general_scenes().items():
        faulty = E.render_batch(V, F, cams, 64, fault)
        try:
            TR.check_against_restatement(V, F, cams, 64, faulty)
            verdicts.append(True)
        except AssertionError:
            verdicts.append(False)
        print(f"{fault}: the stable-only criterion on '{scene}': {'ACCEPTED' if verdicts[-1] else 'rejected'}")
    assert tuple(verdicts) == OLD_VERDICT[fault]


@pytest.mark.parametrize("scene", ["jittered_icosphere", "straddlers", "frame_filling_quad"])
def test_emulation_passes_the_fp64_restatement_on_the_general_scenes(scene):
    """The emulation the GPU is compared with bit for bit on these scenes is itself held by the fp64 criterion."""
    import test_render_gpu as TR
    V, F, cams = E.general_scenes()[scene]
    assert TR.check_against_restatement(V, F, cams, 64, E.render_batch(V, F, cams, 64)) > 0.8 * 64 * 64 * len(cams)
