"""Host side of the HIP image preprocessing (actionmesh_amd/image_preprocess.py; contract: include/actionmesh_amd.h, am_image_*).
No GPU: the tables and the geometry against the code they restate - PIL itself, numpy's float32 expression, the reference's own
functions, transformers' PIL backend - plus the refusals and the drop-in seam.  "Bit-identical" is zero differing
bytes over the whole output; nothing is masked or sampled."""
import ctypes
import importlib.util
import os
import sys
import types

import numpy as np
import pytest
from PIL import Image

from actionmesh_amd import _lib
from actionmesh_amd import image_preprocess as IP

REF = "/root/reference"
HAVE_REF = os.path.isfile(os.path.join(REF, "actionmesh", "preprocessing", "image_processor.py"))
needs_ref = pytest.mark.skipif(not HAVE_REF, reason="reference not present")

# (in width, in height, out width, out height)
RESIZE_CASES = [(614, 614, 256, 256), (100, 100, 256, 256), (1500, 1500, 256, 256), (300, 200, 384, 256), (523, 524, 256, 256),
                (257, 255, 256, 258), (37, 1999, 256, 300), (256, 256, 256, 256), (2, 2, 256, 256)]
DINO_CONFIG = {"crop_size": {"height": 224, "width": 224}, "do_center_crop": True, "do_convert_rgb": True, "do_normalize": True,
               "do_rescale": True, "do_resize": True, "image_mean": [0.485, 0.456, 0.406], "image_std": [0.229, 0.224, 0.225],
               "image_processor_type": "BitImageProcessor", "resample": 3, "rescale_factor": 0.00392156862745098,
               "size": {"shortest_edge": 256}}


def sample_images(w, h, seed):
    """A seeded random image and a black / white step edge (the overshoot of the cubic exercises the clipping)."""
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    edge = np.zeros((h, w, 3), dtype=np.uint8)
    edge[:, w // 2:] = 255
    edge[h // 2:] = 255 - edge[h // 2:]
    return {"random": noise, "step": edge}


def numpy_pass(img, n_out):
    """One horizontal pass with resize_taps, in plain integer arithmetic (the contract's formula)."""
    bounds, k = IP.resize_taps(img.shape[1], n_out)
    out = np.empty((img.shape[0], n_out, img.shape[2]), dtype=np.uint8)
    for i in range(n_out):
        first, count = int(bounds[i, 0]), int(bounds[i, 1])
        acc = np.full((img.shape[0], img.shape[2]), 1 << 21, dtype=np.int32)
        for j in range(count):
            acc = acc + np.int32(k[i, j]) * img[:, first + j].astype(np.int32)
        out[:, i] = np.clip(acc >> 22, 0, 255).astype(np.uint8)
    return out


def numpy_resize(img, out_w, out_h):
    """Horizontal pass into a uint8 image, then the vertical pass on that image."""
    return numpy_pass(numpy_pass(img, out_w).transpose(1, 0, 2), out_h).transpose(1, 0, 2)


@pytest.mark.parametrize("w,h,ow,oh", RESIZE_CASES)
def test_taps_against_pil(w, h, ow, oh):
    for name, img in sample_images(w, h, seed=w * 7919 + h).items():
        want = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BICUBIC))
        got = numpy_resize(img, ow, oh)
        assert got.shape == want.shape
        assert int((got != want).sum()) == 0, (name, int((got != want).sum()))


def test_taps_table_shape_and_packing():
    bounds, k = IP.resize_taps(523, 256)
    assert bounds.shape == (256, 2) and k.shape[0] == 256 and bounds.dtype == np.int32 and k.dtype == np.int32
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= 523).all() and (bounds[:, 1] <= k.shape[1]).all()
    assert (np.abs(k.astype(np.int64).sum(1) - (1 << 22)) <= k.shape[1]).all()          # weights sum to one up to the rounding of each
    packed = IP.pack_taps(523, 256)
    assert packed.dtype == np.int32 and list(packed[:4]) == [523, 256, k.shape[1], 0]
    assert np.array_equal(packed[4: 4 + 512], bounds.reshape(-1)) and np.array_equal(packed[4 + 512:], k.reshape(-1))
    assert IP.resize_taps(523, 256)[1] is k                                            # cached


def test_composite_table_is_the_float32_expression():
    t = IP.composite_table()
    assert t.shape == (256, 256) and t.dtype == np.uint8
    # the reference's expression (image_processor.py:44-52, :144) on an image that holds every (colour, alpha) pair once
    colour, alpha = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    rgb = np.repeat(colour[..., None], 3, axis=2)
    alpha_norm = alpha.astype(np.float32) * (1.0 / 255.0)
    alpha_3ch = alpha_norm[..., np.newaxis]
    bg = np.array([1.0, 1.0, 1.0]).astype(np.float32)
    comp = rgb.astype(np.float32) * (1.0 / 255.0) * alpha_3ch + bg * (1.0 - alpha_3ch)
    want = (comp * 255).astype(np.uint8)
    for c in range(3):
        assert np.array_equal(t, want[..., c])
    assert np.array_equal(t[:, 255], np.arange(256, dtype=np.uint8))                   # opaque: the identity
    assert (t[:, 0] == 255).all()                                                      # transparent: white
    exact = (colour.astype(np.int64) * alpha + 255 * (255 - alpha.astype(np.int64))) // 255
    assert int((t != exact).sum()) == 454                                              # not "any correct blend"


def _ref_module():
    spec = importlib.util.spec_from_file_location("ref_image_processor", os.path.join(REF, "actionmesh", "preprocessing", "image_processor.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@needs_ref
@pytest.mark.parametrize("padding_ratio", [0.1, 0.0, 0.25])
def test_crop_geometry_against_the_reference(padding_ratio):
    import torch
    ref = _ref_module()
    rng = np.random.default_rng(5)
    odd_w = odd_h = 0
    for trial in range(40):
        boxes = []
        for _ in range(int(rng.integers(1, 6))):
            x, y = int(rng.integers(0, 200)), int(rng.integers(0, 200))
            boxes.append((np.int64(x), np.int64(y), np.int64(rng.integers(1, 300 - x)), np.int64(rng.integers(1, 300 - y))))
        image = torch.zeros((3, 300, 300))
        for independent in (False, True):
            ours = IP.crop_geometry(boxes, independent, padding_ratio)
            theirs = boxes if independent else [ref.aggregate_bboxes(boxes)] * len(boxes)
            assert [g[:4] for g in ours] == [tuple(int(v) for v in b) for b in theirs]
            for g, b in zip(ours, theirs):
                out = ref.apply_padding(image, b, padding_ratio, 1.0)
                x, y, w, h, pad_x, pad_y = g
                assert tuple(out.shape) == (3, h + 2 * pad_y, w + 2 * pad_x)
                m = max(w, h)
                odd_w += (m - w) % 2
                odd_h += (m - h) % 2
    assert odd_w > 10 and odd_h > 10            # the by-one-pixel non-square results are among the cases


def test_normalisation_table_against_transformers():
    transformers = pytest.importorskip("transformers")
    proc = transformers.BitImageProcessorPil(do_resize=False, do_center_crop=False, do_rescale=True, do_normalize=True, do_convert_rgb=True,
                                             rescale_factor=DINO_CONFIG["rescale_factor"], image_mean=DINO_CONFIG["image_mean"],
                                             image_std=DINO_CONFIG["image_std"])
    ramp = np.repeat(np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2), 2, axis=0)
    want = np.asarray(proc.preprocess([Image.fromarray(ramp)], return_tensors="np").pixel_values)[0, :, 0, :]
    s = IP.processor_settings(DINO_CONFIG)
    got = IP.normalisation_table(s["rescale_factor"], s["mean"], s["std"])
    assert got.shape == (3, 256) and got.dtype == np.float32 and want.dtype == np.float32
    assert int((got.view(np.uint32) != want.view(np.uint32)).sum()) == 0               # all 768 entries


def test_settings_and_size_rule():
    s = IP.processor_settings(DINO_CONFIG)
    assert (s["shortest_edge"], s["crop_h"], s["crop_w"]) == (256, 224, 224)
    assert IP.resize_plan(614, 614, s) == (256, 256, 16, 16)
    assert IP.resize_plan(523, 524, s) == (256, int(256 * 524 / 523), 16, (int(256 * 524 / 523) - 224) // 2)
    assert IP.resize_plan(700, 400, s) == (448, 256, 112, 16)
    assert IP.resize_plan(300, 701, s) == (256, 598, 16, 187)


@pytest.mark.parametrize("change,field", [({"resample": 2}, "resample"), ({"size": {"height": 256, "width": 256}}, "size"),
                                          ({"do_resize": False}, "do_resize"), ({"do_center_crop": False}, "do_center_crop"),
                                          ({"crop_size": {"shortest_edge": 224}}, "crop_size"),
                                          ({"image_processor_type": "ViTImageProcessor"}, "image_processor_type")])
def test_unsupported_configs_are_refused_by_name(change, field):
    with pytest.raises(ValueError, match=field):
        IP.processor_settings(dict(DINO_CONFIG, **change))


def test_crop_larger_than_the_resized_image_is_refused():
    s = IP.processor_settings(dict(DINO_CONFIG, crop_size={"height": 224, "width": 300}))
    with pytest.raises(ValueError, match="crop_size"):
        IP.resize_plan(512, 512, s)
    assert IP.resize_plan(1024, 512, s)[:2] == (512, 256)


def test_non_rgb_input_without_convert_rgb_is_refused():
    from actionmesh_amd import HipImageEncoder
    enc = HipImageEncoder(pretrained_dino_feature_extractor=dict(DINO_CONFIG, do_convert_rgb=False), preprocess="hip")
    with pytest.raises(ValueError, match="do_convert_rgb"):
        enc.encode_images([Image.new("RGBA", (32, 32))])
    with pytest.raises(ValueError, match="preprocess"):
        HipImageEncoder(preprocess="torchvision")


def test_invalid_alpha_raises_the_references_error():
    H = W = 100                                   # min_count = int(10000 * 0.01) = 100
    ok = np.array([[100, 3, 4, 50, 60, 0, 0, 0]], dtype=np.int32)
    (src,) = IP.sources_from_stats(ok, H, W)
    assert (src.x0, src.y0, src.w, src.h) == (3, 4, 48, 57)
    for count in (99, H * W - 99):                # too little foreground; too little background
        bad = np.array([[100, 3, 4, 50, 60, 0, 0, 0], [count, 3, 4, 50, 60, 0, 0, 0]], dtype=np.int32)
        with pytest.raises(ValueError) as e:
            IP.sources_from_stats(bad, H, W)
        assert str(e.value) == "Invalid alpha channel: insufficient foreground/background"
    if HAVE_REF:
        ref = _ref_module()
        for count in (99, 100, H * W - 100, H * W - 99):
            alpha = np.zeros(H * W, dtype=np.uint8)
            alpha[:count] = 200
            assert IP.alpha_is_valid(count, H * W) == ref.is_valid_alpha(alpha.reshape(H, W))


def test_dropin_rebinds_the_preprocessor_and_the_encoder(monkeypatch):
    """install() + install_preprocess() / uninstall() against a stand-in `actionmesh.pipeline`: the name pipeline.py:97 resolves, and
    the image-encoder node of the composed config."""
    from actionmesh_amd import dropin
    pkg = types.ModuleType("actionmesh")
    pkg.__path__ = []
    P = types.ModuleType("actionmesh.pipeline")

    class ImagePreprocessor:
        pass

    def load_config(config_name, config_dir):
        return {"model": {"scheduler": {"_target_": "a"}, "cf_guidance": {"_target_": "b"},
                          "image_encoder": {"_target_": "actionmesh.model.image_encoder.ImageEncoder", "_partial_": True,
                                            "pretrained_dino_feature_extractor": "w/dinov2", "pretrained_dino_model": "w/dinov2"}}}

    P.ImagePreprocessor, P.load_config = ImagePreprocessor, load_config
    P.ActionMeshDenoiser = type("ActionMeshDenoiser", (), {})
    P.ActionMeshAutoencoder = type("ActionMeshAutoencoder", (), {})
    pkg.pipeline = P
    monkeypatch.setitem(sys.modules, "actionmesh", pkg)
    monkeypatch.setitem(sys.modules, "actionmesh.pipeline", P)
    try:
        dropin.install()
        assert P.ImagePreprocessor is ImagePreprocessor                                # default: left alone
        assert P.load_config("custom.yaml", "/nowhere")["model"]["image_encoder"]["_target_"].endswith(".ImageEncoder")
        dropin.install_preprocess()
        dropin.install_preprocess()                                                    # idempotent
        assert P.ImagePreprocessor is IP.HipImagePreprocessor
        made = P.ImagePreprocessor()                                                   # as pipeline.py:97 calls it
        assert (made.independent_cropping, made.padding_ratio) == (False, 0.1)
        node = P.load_config("custom.yaml", "/nowhere")["model"]["image_encoder"]
        assert node["_target_"] == "actionmesh_amd.image_encoder.HipImageEncoder" and node["preprocess"] == "hip"
        assert node["pretrained_dino_feature_extractor"] == "w/dinov2" and node["_partial_"] is True
        dropin.install()                                                               # a fresh install() takes it back
        assert P.ImagePreprocessor is ImagePreprocessor
        assert "preprocess" not in P.load_config("custom.yaml", "/nowhere")["model"]["image_encoder"]
        dropin.uninstall()
        dropin.install_preprocess()                                                    # on its own: install() with its defaults first
        assert dropin.is_installed() and P.ImagePreprocessor is IP.HipImagePreprocessor
        dropin.uninstall()
        assert P.ImagePreprocessor is ImagePreprocessor and P.load_config is load_config
    finally:
        dropin.uninstall()


def test_cli_flag():
    from actionmesh_amd import cli
    assert cli.split_args([])[0].preprocess == "off"
    ours, rest = cli.split_args(["--preprocess", "hip", "--", "--input", "x"])
    assert ours.preprocess == "hip" and rest == ["--input", "x"]


def test_entry_points_validate_before_launch():
    """Bad arguments are refused on the host (no device is touched): null structs, a window outside its frame, a tap outside its image."""
    lib = _lib.lib()
    for fn in (lib.am_image_alpha_stats, lib.am_image_resample, lib.am_image_materialize):
        assert fn(None, None) != 0 and b"null" in lib.am_last_error()
    frames = (_lib.AmImageFrame * 1)()
    f = frames[0]
    f.src_w = f.src_h = 8
    f.x0, f.y0, f.w, f.h = 4, 0, 8, 8             # runs four columns past the frame
    taps = IP.pack_taps(8, 4)
    a = _lib.AmImageResampleArgs()
    a.src, a.src_bytes, a.src_channels, a.fill, a.n_frames, a.out_w, a.out_h = 4096, 8 * 8 * 3, 3, 255, 1, 4, 4
    a.frames, a.frames_dev = ctypes.addressof(frames), 4096
    a.taps, a.taps_dev, a.taps_len = taps.ctypes.data, 4096, taps.size
    a.out_u8 = 4096
    assert lib.am_image_resample(ctypes.byref(a), None) != 0 and b"window" in lib.am_last_error()
    f.x0 = 0
    f.n_rows = 8
    bad = taps.copy()
    bad[4 + 2 * 3] = 7                            # output 3 would read taps [7, 7 + count) of an 8-sample row
    a.taps = bad.ctypes.data
    assert lib.am_image_resample(ctypes.byref(a), None) != 0 and b"taps" in lib.am_last_error()
    a.taps = taps.ctypes.data
    assert lib.am_image_resample(ctypes.byref(a), None) != 0 and b"workspace" in lib.am_last_error()
