"""Mask refinement on the device (INTEGRATION.md seam S9): the reference's `refine_mask`
(actionmesh/preprocessing/background_removal.py:20-38) - Otsu threshold, 8-connected labelling, removal of components smaller than
`min_size` - on the HIP labelling kernels (csrc/am_components.hip).  The background remover produces its soft mask on the device and
the frame preprocessing (image_preprocess.py) consumes the alpha channel there; with `refine_masks` nothing in between visits the host,
and neither `cv2` nor `skimage` is needed.

What is pinned (tests/test_components_gpu.py, bit for bit): the labelling against `scipy.ndimage.label` with the full 3 x 3 structure,
the threshold against `otsu_threshold` below, and skimage's size rule (a component is removed when its size is < min_size).
UNPINNED: that `cv2.threshold(..., THRESH_OTSU)` returns `otsu_threshold`'s value for every histogram - OpenCV is not installable where
this was written; the loop is a restatement of its getThreshVal_Otsu_8u.

There is no CPU fallback, as in actionbench.py and pointcloud_sampling.py: the library must be loaded and a device present.
"""
import numpy as np
import torch

from . import ops

FLT_EPSILON = float(np.finfo(np.float32).eps)


def otsu_threshold(masks) -> np.ndarray:
    """The threshold of every frame of a uint8 (T, H, W) or (H, W) array, on the host in plain numpy fp64: the loop the header
    (include/actionmesh_amd.h) states and am_mask_refine runs, operation for operation.  Returns int32 (T,) - () for a 2-D input.
    Foreground is `pixel > threshold`.  Documentation and the tests' reference; the product path never calls it."""
    m = masks.detach().cpu().numpy() if isinstance(masks, torch.Tensor) else np.asarray(masks)
    if m.dtype != np.uint8 or m.ndim not in (2, 3):
        raise TypeError(f"otsu_threshold: expected a uint8 (T, H, W) or (H, W) array, got {m.dtype} {m.shape}")
    frames = m[None] if m.ndim == 2 else m
    out = np.zeros(frames.shape[0], np.int32)
    for t, frame in enumerate(frames):
        h = np.bincount(frame.reshape(-1), minlength=256)
        scale = np.float64(1.0) / np.float64(frame.size)
        mu = np.float64(int(sum(i * int(h[i]) for i in range(256)))) * scale
        mu1 = q1 = max_sigma = np.float64(0.0)
        max_val = 0
        for i in range(256):
            p = np.float64(h[i]) * scale
            mu1 = mu1 * q1
            q1 = q1 + p
            q2 = np.float64(1.0) - q1
            if min(q1, q2) < FLT_EPSILON or max(q1, q2) > 1.0 - FLT_EPSILON:
                continue
            mu1 = (mu1 + np.float64(i) * p) / q1
            mu2 = (mu - q1 * mu1) / q2
            sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2)
            if sigma > max_sigma:
                max_sigma, max_val = sigma, i
        out[t] = max_val
    return out[0] if m.ndim == 2 else out


def refine_masks(masks, min_size: int = 200, threshold=None, return_labels: bool = False, return_stats: bool = False):
    """Refine soft masks into clean binary masks on the device.  `masks`: a uint8 (T, H, W) or (H, W) tensor or array, on the device
    or the host (a host input is copied to the current device; a device input is used where it is).  `threshold`: None = Otsu per
    frame, else 0..255 for every frame.  Returns the device uint8 mask (values 0 / 255) shaped like the input; with `return_labels`
    also the int32 labels (0 = background, else 1 + the smallest y * W + x of the pixel's component, small components included);
    with `return_stats` also int32 (T, 4) = [threshold used, foreground pixels, components, components kept] ((4,) for a 2-D input).
    Nothing is read back: the call only enqueues work."""
    m = masks if isinstance(masks, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(masks)))
    if m.dtype != torch.uint8:
        raise TypeError(f"refine_masks: expected a uint8 mask, got {m.dtype}")
    if m.dim() not in (2, 3):
        raise ValueError(f"refine_masks: expected a (T, H, W) or (H, W) mask, got {tuple(m.shape)}")
    single = m.dim() == 2
    m3 = m.unsqueeze(0) if single else m
    if not m3.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("refine_masks: actionmesh_amd kernels need a GPU (no CPU path)")
        m3 = m3.cuda()
    out, labels, stats = ops.mask_refine(m3.contiguous(), min_size=min_size, threshold=-1 if threshold is None else threshold,
                                         return_labels=return_labels, return_stats=return_stats)
    if single:
        out, labels, stats = out[0], (labels[0] if return_labels else None), (stats[0] if return_stats else None)
    res = (out,) + ((labels,) if return_labels else ()) + ((stats,) if return_stats else ())
    return res[0] if len(res) == 1 else res


def refine_mask(mask: np.ndarray, min_size: int = 200) -> np.ndarray:
    """Refine a soft mask into a clean binary mask: the reference's function (background_removal.py:20-38), same name, signature and
    return convention - (H, W) uint8 in, (H, W) uint8 of 0 / 255 out, numpy on both sides - computed by `refine_masks`."""
    return refine_masks(np.asarray(mask), min_size=min_size).cpu().numpy()
