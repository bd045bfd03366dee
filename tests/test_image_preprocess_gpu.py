"""The HIP image preprocessing on the device (csrc/am_image.hip through actionmesh_amd/image_preprocess.py) against the CPU code it
replaces: PIL at run time, the composite table, the reference's recorded `process_images` output on three raw clips
(tests/golden/frames_raw, tools/make_golden_frames_raw.py), the committed DINOv2 input frames (tests/golden/frames), and the encoder's
own "pil" path.  Every comparison is over the whole output and demands zero differing bytes."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from actionmesh_amd import image_preprocess as IP
from actionmesh_amd import ops

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RAW = os.path.join(GOLDEN, "frames_raw")
CLIPS = ["davis_camel", "panda", "kangaroo"]
# (in width, in height, out width, out height)
RESIZE_CASES = [(614, 614, 256, 256), (100, 100, 256, 256), (1500, 1500, 256, 256), (300, 200, 384, 256), (523, 524, 256, 256),
                (257, 255, 256, 258), (37, 1999, 256, 300), (256, 256, 256, 256), (2, 2, 256, 256),
                # tap tables beyond the LDS budget, read from global memory (horizontal, vertical), and the last size that fits
                (2817, 40, 256, 256), (40, 2817, 256, 256), (2816, 40, 256, 256), (40, 2816, 256, 256)]
IMAGE_LDS_BYTES = 48 * 1024         # csrc/am_image.hip
# am_image_alpha_stats sizes its grid for four trips a thread, ceil(npix / (IMAGE_THREADS * 4 * 4)) blocks, and caps it at 256; a trip of
# image_alpha_stats_kernel covers blocks * IMAGE_THREADS * 4 pixels (four pixels a thread)
ALPHA_THREADS, ALPHA_PIXELS_PER_THREAD, ALPHA_TRIPS_UNCAPPED, ALPHA_MAX_BLOCKS = 256, 4, 4, 256
DINO_CONFIG = {"crop_size": {"height": 224, "width": 224}, "do_center_crop": True, "do_convert_rgb": True, "do_normalize": True,
               "do_rescale": True, "do_resize": True, "image_mean": [0.485, 0.456, 0.406], "image_std": [0.229, 0.224, 0.225],
               "image_processor_type": "BitImageProcessor", "resample": 3, "rescale_factor": 0.00392156862745098,
               "size": {"shortest_edge": 256}}


def sample_images(w, h, seed):
    """A seeded random image and a black / white step edge (the same two as the CPU test of the taps)."""
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    edge = np.zeros((h, w, 3), dtype=np.uint8)
    edge[:, w // 2:] = 255
    edge[h // 2:] = 255 - edge[h // 2:]
    return {"random": noise, "step": edge}


def load_clip(clip):
    """(T, H, W, 4) uint8: the parts of a raw clip in frame order."""
    with open(os.path.join(RAW, "expected.json")) as fh:
        parts = json.load(fh)[clip]["parts"]
    return np.concatenate([np.load(os.path.join(RAW, p))["rgba_u8"] for p in parts], axis=0)


def expected(clip, key):
    with open(os.path.join(RAW, "expected.json")) as fh:
        return json.load(fh)[clip][key]


def pil_processor(frames, settings):
    """BitImageProcessor's geometric half with PIL itself: shortest edge, then centre crop (transformers' size rule)."""
    out = []
    for a in frames:
        h, w = a.shape[:2]
        rs_w, rs_h, left, top = IP.resize_plan(w, h, settings)
        r = np.asarray(Image.fromarray(a).resize((rs_w, rs_h), Image.BICUBIC))
        out.append(r[top: top + settings["crop_h"], left: left + settings["crop_w"]])
    return np.stack(out)


@pytest.mark.parametrize("w,h,ow,oh", RESIZE_CASES)
def test_resample_against_pil(w, h, ow, oh):
    images = sample_images(w, h, seed=w * 7919 + h)
    names = sorted(images)
    got = IP.resize_rgb(torch.from_numpy(np.stack([images[n] for n in names])).cuda(), oh, ow).cpu().numpy()
    assert got.shape == (2, oh, ow, 3)
    for i, n in enumerate(names):
        want = np.asarray(Image.fromarray(images[n]).resize((ow, oh), Image.BICUBIC))
        assert int((got[i] != want).sum()) == 0, (n, int((got[i] != want).sum()))


def tap_tables_in_lds(w, h, ow, oh):
    """mirrors use_h / use_v of am_image_resample (csrc/am_image.hip): (horizontal, vertical) table copied to LDS"""
    ks_h, ks_v = int(IP.pack_taps(w, ow)[2]), int(IP.pack_taps(h, oh)[2])
    return ow * (2 + ks_h) * 4 <= IMAGE_LDS_BYTES, oh * (2 + ks_v) * 4 <= IMAGE_LDS_BYTES


def test_resize_cases_reach_both_tap_table_plans():
    """the four threshold cases of RESIZE_CASES select what they are there for: if IMAGE_LDS_BYTES or the tap count moves, this fails
    instead of test_resample_against_pil silently testing the LDS copy four more times"""
    plans = {c: tap_tables_in_lds(*c) for c in RESIZE_CASES}
    assert plans[(2817, 40, 256, 256)] == (False, True) and plans[(40, 2817, 256, 256)] == (True, False)
    assert plans[(2816, 40, 256, 256)] == (True, True) and plans[(40, 2816, 256, 256)] == (True, True)
    assert int(IP.pack_taps(2816, 256)[2]) == 45 and 256 * (2 + 45) * 4 == 48128              # the last size in LDS ...
    assert int(IP.pack_taps(2817, 256)[2]) == 47 and 256 * (2 + 47) * 4 == 50176              # ... and the first one beyond
    assert all(p == (True, True) for c, p in plans.items() if max(c[:2]) < 2816)


def test_resample_both_tables_in_global_memory_and_a_ragged_width():
    """2817 x 2817 -> 255 x 255: both passes read their taps from global memory, and the output width is no multiple of four, so the
    vertical pass stores byte by byte; against PIL, zero differing bytes"""
    w = h = 2817
    ow = oh = 255
    assert tap_tables_in_lds(w, h, ow, oh) == (False, False) and ow % 4 != 0
    images = sample_images(w, h, seed=w * 7919 + h)
    names = sorted(images)
    got = IP.resize_rgb(torch.from_numpy(np.stack([images[n] for n in names])).cuda(), oh, ow).cpu().numpy()
    assert got.shape == (2, oh, ow, 3)
    for i, n in enumerate(names):
        want = np.asarray(Image.fromarray(images[n]).resize((ow, oh), Image.BICUBIC))
        assert int((got[i] != want).sum()) == 0, (n, int((got[i] != want).sum()))


def test_non_square_inputs_through_the_processor_rule():
    """400 x 700, 701 x 300 and 100 x 131 (height x width), each its own geometry, in ONE call - against PIL per image."""
    settings = IP.processor_settings(DINO_CONFIG)
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((400, 700), (701, 300), (100, 131))]
    pix, u8 = IP.rgb_to_pixel_values([torch.from_numpy(f).cuda() for f in frames], settings, return_u8=True)
    want = pil_processor(frames, settings)
    assert int((u8.cpu().numpy() != want).sum()) == 0
    table = IP.normalisation_table(settings["rescale_factor"], settings["mean"], settings["std"])
    want_pix = np.stack([table[c][want[..., c]] for c in range(3)], axis=1)
    assert np.array_equal(pix.cpu().numpy().view(np.uint32), want_pix.view(np.uint32))


def test_composite_of_every_colour_alpha_pair():
    colour, alpha = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    rgba = np.stack([colour, 255 - colour, colour[::-1] ^ 0x55, alpha], axis=-1)          # three different colours per pixel
    src = IP._Source(0, 256, 256, 0, 0, 256, 256)
    frames, _, total = IP._describe([src])
    dev = torch.from_numpy(np.ascontiguousarray(rgba)).cuda()
    comp = torch.from_numpy(IP.composite_table().reshape(-1).copy()).cuda()
    out = ops.image_materialize(dev.reshape(-1), 4, frames, IP._upload_frames(frames, dev.device), total, composite=comp, fill=255)
    got = out[: 256 * 256 * 3].view(256, 256, 3).cpu().numpy()
    table = IP.composite_table()
    want = np.stack([table[rgba[..., c], alpha] for c in range(3)], axis=-1)
    assert int((got != want).sum()) == 0


def test_alpha_stats_against_numpy():
    rng = np.random.default_rng(3)
    for shape in ((3, 64, 80), (2, 37, 53), (1, 512, 512)):
        rgba = rng.integers(0, 256, shape + (4,), dtype=np.uint8)
        rgba[..., 3] = np.where(rng.random(shape) < 0.6, 0, rgba[..., 3])
        rgba[:, :5] = 0
        rgba[:, :, :7] = 0
        rgba[0, -3:] = 0
        got = ops.image_alpha_stats(torch.from_numpy(rgba).cuda()).cpu().numpy()
        for t in range(shape[0]):
            a = rgba[t, ..., 3]
            ys, xs = np.nonzero(a > 0)
            assert list(got[t]) == [int((a > 127).sum()), xs.min(), ys.min(), xs.max(), ys.max(), 0, 0, 0]
    empty = np.zeros((1, 16, 16, 4), dtype=np.uint8)
    assert list(ops.image_alpha_stats(torch.from_numpy(empty).cuda()).cpu().numpy()[0][:5]) == [0, 2 ** 31 - 1, 2 ** 31 - 1, -1, -1]


@pytest.mark.parametrize("H,W", [(1024, 1025), (1023, 1027)], ids=["vector-loads", "scalar-loads"])
def test_alpha_stats_fifth_trip_on_the_capped_grid(H, W):
    """The grid of am_image_alpha_stats is sized so that a thread of image_alpha_stats_kernel makes up to four trips of its
    grid-stride loop, until the cap of 256 blocks binds: beyond 256 x 4096 = 1 048 576 pixels a frame the loop runs a fifth trip,
    which no smaller frame does (512 x 512 is 64 blocks and four trips).  Frame 0 is random; every alpha > 0 of frame 1 lies beyond
    pixel 1 048 576, that is in the fifth trip alone, one of them in the very last column of the last row, so a dropped or
    misindexed fifth trip changes the count and all four bounds"""
    npix = H * W
    # mirrors the launch of am_image_alpha_stats: min(ceil(npix / (IMAGE_THREADS * 4 * 4)), 256) blocks ...
    blocks = min(-(-npix // (ALPHA_THREADS * ALPHA_PIXELS_PER_THREAD * ALPHA_TRIPS_UNCAPPED)), ALPHA_MAX_BLOCKS)
    # ... and the loop of image_alpha_stats_kernel: step = gridDim.x * IMAGE_THREADS * 4 pixels
    step = blocks * ALPHA_THREADS * ALPHA_PIXELS_PER_THREAD
    four_trips = ALPHA_TRIPS_UNCAPPED * step                # the pixels that the first four trips cover
    assert blocks == ALPHA_MAX_BLOCKS and step == 262_144 and four_trips == 1_048_576
    assert -(-npix // step) == 5 > ALPHA_TRIPS_UNCAPPED
    assert (npix % 4 == 0) == (W == 1025)                   # vector loads need a multiple of four pixels a frame
    rng = np.random.default_rng(H)
    rgba = rng.integers(0, 256, (2, H, W, 4), dtype=np.uint8)
    rgba[0, ..., 3] = np.where(rng.random((H, W)) < 0.6, 0, rgba[0, ..., 3])
    rgba[0, :5] = 0
    rgba[0, :, :7] = 0
    a1 = np.where(rng.random(npix) < 0.5, 0, rgba[1, ..., 3].reshape(-1))
    a1[:four_trips] = 0                                     # nothing in trips one to four: what is left is the last rows only
    a1[four_trips] = 90                                     # the first pixel of the fifth trip ...
    a1[-1] = 200                                            # ... and the last column of the last row
    rgba[1, ..., 3] = a1.reshape(H, W)
    assert (np.nonzero(a1)[0] >= four_trips).all() and np.count_nonzero(a1) > 400
    got = ops.image_alpha_stats(torch.from_numpy(rgba).cuda()).cpu().numpy()
    for t in range(2):
        a = rgba[t, ..., 3]
        ys, xs = np.nonzero(a > 0)
        assert list(got[t]) == [int((a > 127).sum()), xs.min(), ys.min(), xs.max(), ys.max(), 0, 0, 0], t
    assert got[1][3] == W - 1 and got[1][4] == H - 1 and got[1][2] == four_trips // W


def test_invalid_alpha_raises_on_the_device_path():
    opaque = np.full((2, 64, 64, 4), 255, dtype=np.uint8)
    with pytest.raises(ValueError) as e:
        IP.HipImagePreprocessor().process_frames(torch.from_numpy(opaque).cuda())
    assert str(e.value) == "Invalid alpha channel: insufficient foreground/background"


@pytest.mark.parametrize("independent", [False, True])
@pytest.mark.parametrize("clip", CLIPS)
def test_process_frames_against_the_reference(clip, independent):
    want = expected(clip, "independent" if independent else "shared")
    out = IP.HipImagePreprocessor(independent_cropping=independent).process_frames(torch.from_numpy(load_clip(clip)).cuda())
    assert [[int(f.shape[1]), int(f.shape[0])] for f in out] == want["sizes"]
    h = hashlib.sha256()
    for f in out:
        assert f.dtype == torch.uint8 and f.shape[2] == 3
        h.update(f.cpu().numpy().tobytes())
    assert h.hexdigest() == want["sha256"]


def test_process_images_returns_the_references_pil_frames():
    clip = load_clip("kangaroo")
    out = IP.HipImagePreprocessor().process_images([Image.fromarray(f) for f in clip])
    want = expected("kangaroo", "shared")
    assert all(isinstance(im, Image.Image) and im.mode == "RGB" for im in out)
    assert [list(im.size) for im in out] == want["sizes"]
    h = hashlib.sha256()
    for im in out:
        h.update(np.asarray(im).tobytes())
    assert h.hexdigest() == want["sha256"]


@pytest.mark.parametrize("clip", CLIPS)
def test_raw_frames_to_the_uint8_crop_and_pixel_values(clip):
    settings = IP.processor_settings(DINO_CONFIG)
    raw = torch.from_numpy(load_clip(clip)).cuda()
    pix, u8 = IP.frames_to_pixel_values(raw, settings, return_u8=True)
    u8 = u8.cpu().numpy()
    if clip == "kangaroo":                        # the non-square case (523 x 524): PIL applied to the process_frames output
        frames = [f.cpu().numpy() for f in IP.HipImagePreprocessor().process_frames(raw)]
        assert frames[0].shape[:2] == (524, 523)
        want = pil_processor(frames, settings)
    else:
        want = np.load(os.path.join(GOLDEN, "frames", f"{clip}_16x224.npz"))["rgb_u8"]
    assert u8.shape == want.shape == (16, 224, 224, 3)
    assert int((u8 != want).sum()) == 0
    table = IP.normalisation_table(settings["rescale_factor"], settings["mean"], settings["std"])
    want_pix = np.stack([table[c][u8[..., c]] for c in range(3)], axis=1)
    got_pix = pix.cpu().numpy()
    assert got_pix.shape == (16, 3, 224, 224) and got_pix.dtype == np.float32
    assert np.array_equal(got_pix.view(np.uint32), want_pix.view(np.uint32))
    # without the optional uint8 output the pixels are the same
    assert torch.equal(IP.frames_to_pixel_values(raw, settings), pix)


@pytest.mark.parametrize("clip", ["kangaroo", "panda"])
def test_independent_cropping_does_not_depend_on_the_grouping(clip):
    settings = IP.processor_settings(DINO_CONFIG)
    raw = torch.from_numpy(load_clip(clip)).cuda()
    pix, u8 = IP.frames_to_pixel_values(raw, settings, independent_cropping=True, return_u8=True)
    pre = IP.HipImagePreprocessor(independent_cropping=True)
    frames = pre.process_frames(raw)
    want = pil_processor([f.cpu().numpy() for f in frames], settings)
    assert int((u8.cpu().numpy() != want).sum()) == 0
    for t in range(raw.shape[0]):
        p1, u1 = IP.frames_to_pixel_values(raw[t: t + 1], settings, independent_cropping=True, return_u8=True)
        assert torch.equal(u1[0], u8[t]) and torch.equal(p1[0], pix[t])
        (f1,) = pre.process_frames(raw[t: t + 1])
        assert torch.equal(f1, frames[t])


def test_encoder_context_from_raw_frames_equals_the_pil_path(tmp_path):
    """A small seeded DINOv2: encode_frames(raw) - both halves on the device - against encode_images on the "pil" path fed the PIL
    frames of process_images, and against encode_images on the "hip" path.  Same kernels, same input bits: bitwise-equal context."""
    pytest.importorskip("transformers")
    from actionmesh_amd import HipImageEncoder
    from oracle import dinov2_oracle as DO
    cfg = DO.DinoConfig(num_hidden_layers=2)
    sd = DO.synthetic_state_dict(cfg, seed=3)
    with open(tmp_path / "preprocessor_config.json", "w") as fh:
        json.dump(DINO_CONFIG, fh)
    clip = load_clip("kangaroo")
    kw = dict(pretrained_dino_feature_extractor=str(tmp_path), config=dict(num_hidden_layers=2), state_dict=sd)
    hip = HipImageEncoder(preprocess="hip", **kw).to("cuda:0")
    pil = HipImageEncoder(**kw).to("cuda:0")
    assert pil.preprocess == "pil"
    ctx_raw = hip.encode_frames(torch.from_numpy(clip))
    pil_frames = IP.HipImagePreprocessor(device="cuda:0").process_images([Image.fromarray(f) for f in clip])
    ctx_pil = pil.encode_images(pil_frames)
    ctx_hip = hip.encode_images(pil_frames)
    assert ctx_raw.shape == (16, 257, 1024) and bool(torch.isfinite(ctx_raw).all())
    assert torch.equal(ctx_raw, ctx_pil)
    assert torch.equal(ctx_hip, ctx_pil)
    assert torch.equal(pil.encode_frames(torch.from_numpy(clip)), ctx_pil)      # encode_frames is on the device whatever `preprocess` is
