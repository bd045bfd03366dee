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
                (257, 255, 256, 258), (37, 1999, 256, 300), (256, 256, 256, 256), (2, 2, 256, 256)]
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
