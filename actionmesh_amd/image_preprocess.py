"""Image preprocessing in front of the context encoder on HIP, bit-identical to the CPU code it replaces (seam S8).

Two CPU stages stand between the video frames and DINOv2 in the reference:
  1. `ImagePreprocessor.process_images` (actionmesh/preprocessing/image_processor.py:124-146): validity of the alpha mask (:15-23),
     composite on white (:44-52), bounding box of alpha > 0 (:57-65), shared or per-frame box (:70-78), square padding (:81-101);
  2. transformers' `BitImageProcessor` on its PIL backend (image_encoder.py:48-51): resize of the shortest edge (PIL's antialiased
     bicubic), centre crop, rescale, normalise.
Both are integer or table arithmetic from end to end, so the device version is exact.  The contract - what each table holds, how PIL
samples - is stated at `am_image_alpha_stats` / `am_image_resample` / `am_image_materialize` in include/actionmesh_amd.h; this module
is its host side: the tables (built in numpy, cached), the geometry (plain integers), and the orchestration of the three entry points.
The one device-to-host read is the T rows of alpha statistics: the reference raises on them and every size depends on them.

    HipImagePreprocessor(independent_cropping, padding_ratio)    the reference's dataclass: process_images(list[PIL]) -> list[PIL],
                                                                 process_frames(rgba_u8 device) -> device uint8 frames
    frames_to_pixel_values(rgba_u8, processor_config)            raw RGBA frames -> pixel_values (T, 3, ch, cw), both stages at once:
                                                                 the composited square frames are never written
    rgb_to_pixel_values(frames, processor_config)                stage 2 alone, on RGB frames already processed
There is no CPU path: without the library these raise.
"""
from __future__ import annotations

import ctypes as C
import functools
import json
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib as L
from . import ops

INVALID_ALPHA = "Invalid alpha channel: insufficient foreground/background"      # the reference's message (image_processor.py:41)
PRECISION_BITS = 22            # PIL's fixed point for 8-bit images
FILL = 255                     # the reference pads with its background colour, white


# ---- tables -------------------------------------------------------------------------------------------------------------------------
def _cubic(x: np.ndarray) -> np.ndarray:
    """Keys' cubic with a = -0.5 in fp64, Horner form."""
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    far = (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


@functools.lru_cache(maxsize=256)
def resize_taps(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """One 1-D pass of the antialiased bicubic resample from `n_in` to `n_out` samples: (bounds (n_out, 2) int32 = first tap and tap
    count of every output, k (n_out, ksize) int32 = the 22-bit fixed-point weights, zero beyond the count).  Built in fp64; depends
    on (n_in, n_out) only; cached (the arrays are read-only)."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resize_taps: sizes must be positive, got {n_in} -> {n_out}")
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(np.ceil(support)) * 2 + 1
    centre = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    first = np.maximum((centre - support + 0.5).astype(np.int64), 0)              # the cast truncates
    last = np.minimum((centre + support + 0.5).astype(np.int64), n_in)
    count = last - first
    inv = 1.0 / fs
    w = np.zeros((n_out, ksize), dtype=np.float64)
    total = np.zeros(n_out, dtype=np.float64)
    for j in range(ksize):                      # the sum runs over the taps in order, as a scalar loop would
        wj = np.where(j < count, _cubic((j + first - centre + 0.5) * inv), 0.0)
        w[:, j] = wj
        total = total + wj
    w = np.where(total[:, None] != 0.0, w / np.where(total == 0.0, 1.0, total)[:, None], w)
    k = (w * float(1 << PRECISION_BITS) + np.where(w < 0.0, -0.5, 0.5)).astype(np.int64).astype(np.int32)      # truncation
    k[np.arange(ksize)[None, :] >= count[:, None]] = 0
    bounds = np.stack([first, count], axis=1).astype(np.int32)
    bounds.setflags(write=False)
    k.setflags(write=False)
    return bounds, k


def pack_taps(n_in: int, n_out: int) -> np.ndarray:
    """The table as am_image_resample reads it: {in, out, ksize, 0, (first, count) x out, k[out][ksize]} int32."""
    bounds, k = resize_taps(n_in, n_out)
    return np.concatenate([np.array([n_in, n_out, k.shape[1], 0], dtype=np.int32), bounds.reshape(-1), k.reshape(-1)])


@functools.lru_cache(maxsize=1)
def composite_table() -> np.ndarray:
    """uint8 (256, 256) indexed [colour, alpha]: the float32 expression of image_processor.py:44-52 on a white background, times 255,
    truncated (:144) - evaluated by numpy itself over all 65536 pairs, so it is right by construction."""
    colour = np.arange(256, dtype=np.uint8)[:, None]
    alpha = np.arange(256, dtype=np.uint8)[None, :]
    alpha_norm = alpha.astype(np.float32) * (1.0 / 255.0)
    bg = np.array([1.0]).astype(np.float32)
    comp = colour.astype(np.float32) * (1.0 / 255.0) * alpha_norm + bg * (1.0 - alpha_norm)
    table = (comp * 255).astype(np.uint8)
    table.setflags(write=False)
    return table


def normalisation_table(rescale_factor: float = 1.0 / 255.0, mean: Sequence[float] = (0.485, 0.456, 0.406),
                        std: Sequence[float] = (0.229, 0.224, 0.225)) -> np.ndarray:
    """fp32 (3, 256): t[c, v] = (fp32(v * rescale_factor) - fp32(mean[c])) / fp32(std[c]); the product in fp64, the rest in fp32 - the
    arithmetic of BitImageProcessor's PIL backend on an 8-bit image."""
    v = (np.arange(256, dtype=np.float64) * float(rescale_factor)).astype(np.float32)
    m = np.asarray(mean, dtype=np.float32).reshape(3, 1)
    s = np.asarray(std, dtype=np.float32).reshape(3, 1)
    return ((v[None, :] - m) / s).astype(np.float32)


# ---- geometry -----------------------------------------------------------------------------------------------------------------------
def alpha_is_valid(fg_count: int, n_pixels: int, min_ratio: float = 0.01) -> bool:
    """image_processor.py:15-23 from the count of alpha > 127."""
    min_count = int(n_pixels * min_ratio)
    return n_pixels - fg_count >= min_count and fg_count >= min_count


def crop_geometry(bboxes: Sequence[Tuple[int, int, int, int]], independent_cropping: bool = False,
                  padding_ratio: float = 0.1) -> List[Tuple[int, int, int, int, int, int]]:
    """Per frame (x, y, w, h, pad_x, pad_y) from the frames' (x, y, w, h) boxes of alpha > 0: the union box unless cropped
    independently (image_processor.py:70-78), then the padding of :93-97.  The padded frame is (w + 2 pad_x) x (h + 2 pad_y)."""
    boxes = [tuple(int(v) for v in b) for b in bboxes]
    if not independent_cropping:
        x0, y0 = min(b[0] for b in boxes), min(b[1] for b in boxes)
        x1, y1 = max(b[0] + b[2] for b in boxes), max(b[1] + b[3] for b in boxes)
        boxes = [(x0, y0, x1 - x0, y1 - y0)] * len(boxes)
    out = []
    for x, y, w, h in boxes:
        m = max(w, h)
        pad = int(m * padding_ratio)
        out.append((x, y, w, h, pad + (m - w) // 2, pad + (m - h) // 2))
    return out


_SETTING_DEFAULTS = dict(do_resize=True, do_center_crop=True, do_rescale=True, do_normalize=True, do_convert_rgb=True, resample=3,
                         rescale_factor=1.0 / 255.0)


def processor_settings(config: Union[str, Dict]) -> Dict:
    """The fields of a `preprocessor_config.json` (a path to the file or its directory, or the dict) this module implements, validated:
    anything it does not implement is refused by name."""
    if isinstance(config, (str, os.PathLike)):
        path = os.fspath(config)
        if os.path.isdir(path):
            path = os.path.join(path, "preprocessor_config.json")
        with open(path) as fh:
            config = json.load(fh)
    cfg = dict(_SETTING_DEFAULTS)
    cfg.update({k: v for k, v in config.items() if v is not None})
    kind = cfg.get("image_processor_type", "BitImageProcessor")
    if not str(kind).startswith("BitImageProcessor"):
        raise ValueError(f"image_preprocess: image_processor_type={kind!r} is not supported (BitImageProcessor only)")
    for flag in ("do_resize", "do_center_crop"):
        if not cfg[flag]:
            raise ValueError(f"image_preprocess: {flag}=False is not supported")
    if int(cfg["resample"]) != 3:
        raise ValueError(f"image_preprocess: resample={cfg['resample']!r} is not supported (3 = bicubic only)")
    size = cfg.get("size")
    if isinstance(size, int):
        size = {"shortest_edge": size}
    if not isinstance(size, dict) or set(size) != {"shortest_edge"}:
        raise ValueError(f"image_preprocess: size={cfg.get('size')!r} is not supported (shortest_edge only)")
    crop = cfg.get("crop_size")
    if isinstance(crop, int):
        crop = {"height": crop, "width": crop}
    if not isinstance(crop, dict) or set(crop) != {"height", "width"}:
        raise ValueError(f"image_preprocess: crop_size={cfg.get('crop_size')!r} is not supported (height and width only)")
    mean, std = cfg.get("image_mean"), cfg.get("image_std")
    if cfg["do_normalize"] and (mean is None or std is None or len(mean) != 3 or len(std) != 3):
        raise ValueError("image_preprocess: do_normalize needs image_mean and image_std of three channels")
    return dict(shortest_edge=int(size["shortest_edge"]), crop_h=int(crop["height"]), crop_w=int(crop["width"]),
                rescale_factor=float(cfg["rescale_factor"]) if cfg["do_rescale"] else 1.0,
                mean=tuple(float(v) for v in mean) if cfg["do_normalize"] else (0.0, 0.0, 0.0),
                std=tuple(float(v) for v in std) if cfg["do_normalize"] else (1.0, 1.0, 1.0),
                do_convert_rgb=bool(cfg["do_convert_rgb"]))


def resize_plan(in_w: int, in_h: int, settings: Dict) -> Tuple[int, int, int, int]:
    """(resized width, resized height, crop left, crop top) of an in_w x in_h image: transformers' shortest-edge rule and centre crop."""
    S, ch, cw = settings["shortest_edge"], settings["crop_h"], settings["crop_w"]
    if in_w <= in_h:
        rs_w, rs_h = S, int(S * in_h / in_w)
    else:
        rs_w, rs_h = int(S * in_w / in_h), S
    if ch > rs_h or cw > rs_w:
        raise ValueError(f"image_preprocess: crop_size {ch} x {cw} (height x width) is larger than the resized image {rs_h} x {rs_w}")
    return rs_w, rs_h, (rs_w - cw) // 2, (rs_h - ch) // 2


# ---- frame descriptions ------------------------------------------------------------------------------------------------------------
@dataclass
class _Source:
    """One stored frame and the window of it a padded image is made of."""
    src_offset: int
    src_w: int
    src_h: int
    x0: int
    y0: int
    w: int
    h: int
    pad_x: int = 0
    pad_y: int = 0

    @property
    def size(self) -> Tuple[int, int]:
        return self.w + 2 * self.pad_x, self.h + 2 * self.pad_y


def _describe(sources: Sequence[_Source], plans: Optional[Sequence[Tuple[int, int, int, int]]] = None, out_hw: Optional[Tuple[int, int]] = None):
    """ctypes array of AmImageFrame (+ the int32 tap tables of `plans`, every (in, out) pair once).  Without plans: the frames of
    am_image_materialize, laid out back to back at 16-byte aligned offsets; returns (frames, None, total bytes)."""
    frames = (L.AmImageFrame * len(sources))()
    tables: Dict[Tuple[int, int], int] = {}
    chunks: List[np.ndarray] = []
    length = 0

    def table(n_in: int, n_out: int) -> int:
        nonlocal length
        if (n_in, n_out) not in tables:
            t = pack_taps(n_in, n_out)
            tables[(n_in, n_out)] = length
            chunks.append(t)
            length += t.size
        return tables[(n_in, n_out)]

    dst = 0
    for i, s in enumerate(sources):
        f = frames[i]
        f.src_offset, f.src_w, f.src_h = s.src_offset, s.src_w, s.src_h
        f.x0, f.y0, f.w, f.h, f.pad_x, f.pad_y = s.x0, s.y0, s.w, s.h, s.pad_x, s.pad_y
        in_w, in_h = s.size
        if plans is None:
            f.dst_offset = dst
            dst += ops.round_up(in_w * in_h * 3, 16)
            continue
        rs_w, rs_h, left, top = plans[i]
        out_h, out_w = out_hw
        f.htab, f.vtab, f.left, f.top = table(in_w, rs_w), table(in_h, rs_h), left, top
        vb = resize_taps(in_h, rs_h)[0][top: top + out_h]
        f.row_lo = int(vb[:, 0].min())
        f.n_rows = int((vb[:, 0] + vb[:, 1]).max()) - f.row_lo
    if plans is None:
        return frames, None, dst
    return frames, np.ascontiguousarray(np.concatenate(chunks)), 0


_device_tables: Dict[Tuple, torch.Tensor] = {}


def _on_device(key: Tuple, device: torch.device, make) -> torch.Tensor:
    """A small host table uploaded once per device."""
    k = (str(device),) + key
    if k not in _device_tables:
        if len(_device_tables) > 64:
            _device_tables.clear()
        _device_tables[k] = torch.from_numpy(np.array(make(), order="C")).to(device)
    return _device_tables[k]


def _upload_frames(frames, device: torch.device) -> torch.Tensor:
    return torch.frombuffer(bytearray(bytes(frames)), dtype=torch.uint8).to(device)


def _need_u8(t: torch.Tensor, channels: int, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{what}: actionmesh_amd kernels need a device tensor (no CPU path)")
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != channels or t.numel() == 0:
        raise ValueError(f"{what}: expected non-empty (T, H, W, {channels}) uint8 frames, got {tuple(t.shape)} {t.dtype}")
    return t.contiguous()


def _run_resample(src: torch.Tensor, channels: int, sources: Sequence[_Source], plans, out_h: int, out_w: int,
                  norm: Optional[np.ndarray], want_u8: bool):
    dev = src.device
    frames, taps, _ = _describe(sources, plans, (out_h, out_w))
    comp = _on_device(("composite",), dev, lambda: composite_table().reshape(-1)) if channels == 4 else None
    norm_dev = None if norm is None else _on_device(("norm", norm.tobytes()), dev, lambda: norm.reshape(-1))
    taps_dev = _on_device(("taps", taps.tobytes()), dev, lambda: taps)
    return ops.image_resample(src.reshape(-1), channels, frames, _upload_frames(frames, dev), taps, taps_dev, out_h, out_w, composite=comp,
                              fill=FILL, norm_table=norm_dev, want_u8=want_u8)


def resize_rgb(rgb_u8: torch.Tensor, out_h: int, out_w: int) -> torch.Tensor:
    """PIL's `Image.resize((out_w, out_h), BICUBIC)` of every frame of a device tensor (T, H, W, 3) uint8 -> (T, out_h, out_w, 3)."""
    rgb_u8 = _need_u8(rgb_u8, 3, "resize_rgb")
    T, H, W, _ = rgb_u8.shape
    sources = [_Source(t * H * W * 3, W, H, 0, 0, W, H) for t in range(T)]
    if (H * W * 3) % 4:                        # frame offsets must be multiples of 4: lay the frames out again
        stride = ops.round_up(H * W * 3, 4)
        flat = torch.zeros((T, stride), dtype=torch.uint8, device=rgb_u8.device)
        flat[:, : H * W * 3] = rgb_u8.reshape(T, -1)
        rgb_u8, sources = flat, [_Source(t * stride, W, H, 0, 0, W, H) for t in range(T)]
    return _run_resample(rgb_u8, 3, sources, [(int(out_w), int(out_h), 0, 0)] * T, int(out_h), int(out_w), None, True)[1]


def _settings(processor_config: Union[str, Dict]) -> Dict:
    """Validated settings: what processor_settings returned is passed through."""
    if isinstance(processor_config, dict) and "crop_h" in processor_config and "shortest_edge" in processor_config:
        return processor_config
    return processor_settings(processor_config)


def _normalisation(settings: Dict) -> np.ndarray:
    return normalisation_table(settings["rescale_factor"], settings["mean"], settings["std"])


def rgb_to_pixel_values(frames: Union[torch.Tensor, Sequence[torch.Tensor]], processor_config: Union[str, Dict], return_u8: bool = False):
    """BitImageProcessor.preprocess of RGB frames on the device: a tensor (T, H, W, 3) uint8, or a sequence of (H_t, W_t, 3) uint8
    tensors of any sizes.  Returns pixel_values (T, 3, ch, cw) fp32 - and with `return_u8` also the uint8 crop (T, ch, cw, 3)."""
    settings = _settings(processor_config)
    whole = None
    if isinstance(frames, torch.Tensor):
        whole = _need_u8(frames, 3, "rgb_to_pixel_values")
        frames = list(whole)
    if not frames:
        raise ValueError("rgb_to_pixel_values: no frames")
    dev = frames[0].device
    sources, offset = [], 0
    for f in frames:
        f = _need_u8(f[None], 3, "rgb_to_pixel_values")[0]
        sources.append(_Source(offset, f.shape[1], f.shape[0], 0, 0, f.shape[1], f.shape[0]))
        offset += ops.round_up(f.numel(), 4)
    if len({s.size for s in sources}) == 1 and sources[0].src_w * sources[0].src_h * 3 % 4 == 0:
        flat = (whole if whole is not None else torch.stack(list(frames))).reshape(-1)
    else:
        flat = torch.zeros((offset,), dtype=torch.uint8, device=dev)
        for s, f in zip(sources, frames):
            flat[s.src_offset: s.src_offset + f.numel()] = f.reshape(-1)
    plans = [resize_plan(*s.size, settings) for s in sources]
    pix, u8 = _run_resample(flat, 3, sources, plans, settings["crop_h"], settings["crop_w"], _normalisation(settings), return_u8)
    return (pix, u8) if return_u8 else pix


def sources_from_stats(stats: np.ndarray, height: int, width: int, independent_cropping: bool = False,
                       padding_ratio: float = 0.1) -> List[_Source]:
    """The T rows of am_image_alpha_stats (host) -> the frames' crop windows: the reference's validity check (it raises the
    reference's ValueError) and crop geometry.  Frame t is stored at t * height * width * 4 bytes."""
    boxes = []
    for t in range(len(stats)):
        count, x0, y0, x1, y1 = (int(v) for v in stats[t][:5])
        if not alpha_is_valid(count, height * width):
            raise ValueError(INVALID_ALPHA)
        if x1 < x0:
            raise ValueError(f"image_preprocess: frame {t} has no pixel with alpha > 0")
        boxes.append((x0, y0, x1 - x0 + 1, y1 - y0 + 1))
    geo = crop_geometry(boxes, independent_cropping, padding_ratio)
    return [_Source(t * height * width * 4, width, height, *g) for t, g in enumerate(geo)]


def _crop_sources(rgba_u8: torch.Tensor, independent_cropping: bool, padding_ratio: float) -> List[_Source]:
    """Alpha statistics on the device, then ONE read of the T rows."""
    T, H, W, _ = rgba_u8.shape
    return sources_from_stats(ops.image_alpha_stats(rgba_u8).cpu().numpy(), H, W, independent_cropping, padding_ratio)


def frames_to_pixel_values(rgba_u8: torch.Tensor, processor_config: Union[str, Dict], independent_cropping: bool = False,
                           padding_ratio: float = 0.1, return_u8: bool = False):
    """Raw frames to DINOv2 input in one go: rgba_u8 (T, H, W, 4) uint8 on the device -> pixel_values (T, 3, ch, cw) fp32, bit-identical
    to `BitImageProcessor(ImagePreprocessor.process_images(frames))` - with `return_u8` also the uint8 crop (T, ch, cw, 3)."""
    settings = _settings(processor_config)
    rgba_u8 = _need_u8(rgba_u8, 4, "frames_to_pixel_values")
    sources = _crop_sources(rgba_u8, independent_cropping, padding_ratio)
    plans = [resize_plan(*s.size, settings) for s in sources]
    pix, u8 = _run_resample(rgba_u8, 4, sources, plans, settings["crop_h"], settings["crop_w"], _normalisation(settings), return_u8)
    return (pix, u8) if return_u8 else pix


@dataclass(eq=False)
class HipImagePreprocessor:
    """The reference's `ImagePreprocessor` (image_processor.py:104-146; same two fields, same `process_images`) on the device."""

    independent_cropping: bool = False
    padding_ratio: float = 0.1
    device: str = "cuda"

    def process_frames(self, rgba_u8: torch.Tensor) -> List[torch.Tensor]:
        """rgba_u8 (T, H, W, 4) uint8 on the device -> T device tensors (h_t, w_t, 3) uint8: composited on white, cropped, padded.
        With the shared box all T have one size; cropped independently each has its own (they are views of one buffer)."""
        rgba_u8 = _need_u8(rgba_u8, 4, "HipImagePreprocessor.process_frames")
        sources = _crop_sources(rgba_u8, self.independent_cropping, self.padding_ratio)
        frames, _, total = _describe(sources)
        dev = rgba_u8.device
        comp = _on_device(("composite",), dev, lambda: composite_table().reshape(-1))
        out = ops.image_materialize(rgba_u8.reshape(-1), 4, frames, _upload_frames(frames, dev), total, composite=comp, fill=FILL)
        return [out[f.dst_offset: f.dst_offset + s.size[0] * s.size[1] * 3].view(s.size[1], s.size[0], 3) for f, s in zip(frames, sources)]

    def process_images(self, frames: List) -> List:
        """list[PIL.Image] -> list[PIL.Image] (RGB), the reference's contract: the pipeline's other consumers take PIL images."""
        from PIL import Image
        arrays = [np.ascontiguousarray(f if f.mode == "RGBA" else f.convert("RGBA")) for f in frames]
        out: List = [None] * len(arrays)
        groups: Dict[Tuple, List[int]] = {}
        for i, a in enumerate(arrays):
            groups.setdefault(a.shape, []).append(i)
        if not self.independent_cropping and len(groups) > 1:
            raise ValueError("HipImagePreprocessor.process_images: a shared crop needs frames of one size")
        for idx in groups.values():
            dev_frames = self.process_frames(torch.from_numpy(np.stack([arrays[i] for i in idx])).to(self.device))
            if len({tuple(f.shape) for f in dev_frames}) == 1:
                host = list(torch.stack(dev_frames).cpu().numpy())
            else:
                host = [f.cpu().numpy() for f in dev_frames]
            for i, h in zip(idx, host):
                out[i] = Image.fromarray(h)
        return out
