"""The preview video of the reference CLI (`grid_normal.mp4`: the input frames beside three views of the animated mesh as normal
maps) without PyTorch3D (INTEGRATION.md seam S6).

The reference renders it through actionmesh/render/{visualizer,renderer,cameras,utils}.py, all PyTorch3D, and skips it when
`import pytorch3d` fails (inference/video_to_animated_mesh.py:26-37, 108-118).  Here:

  * `uniform_cameras` restates cameras.py:57-139 (`get_uniform_camera`) as plain tensors;
  * `HipRenderer.render_normals` draws every (frame, camera) image of a call with am_render_normals (csrc/am_raster.hip): the
    reference's 2x supersampled hard raster, interpolated vertex normals and `soft_normal_shading` (renderer.py:58, 119-185);
  * `HipVisualizer.render` mirrors `ActionMeshVisualizer.render` (visualizer.py:84-152) and `save_multiview_video_grid`
    (utils.py:117-174): the grid video at 12 fps through imageio when it is importable, else a lossless animated PNG;
  * `install_hook` / `render_captured` let `python -m actionmesh_amd.cli --render` draw it after the unmodified reference script
    has run: the script's own `load_frames` and `save_deformation` are wrapped to keep the input frames, the meshes and the output
    directory.

Parity with PyTorch3D is unpinned (PyTorch3D is not installable offline); the conventions written in include/actionmesh_amd.h
(am_render_normals) are the contract the tests hold.
"""
from __future__ import annotations

import logging
import math
import os
from itertools import cycle
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

logger = logging.getLogger(__name__)

FPS = 12
VISUALIZER_CAMERAS = ("U000", "U004", "U008")


# ---- cameras (cameras.py) -----------------------------------------------------------------------------------------------------
def look_at_rotation(camera_position: torch.Tensor, up=(0.0, 1.0, 0.0)) -> torch.Tensor:
    """PyTorch3D's `look_at_rotation` towards the origin: (N, 3) positions -> (N, 3, 3) R whose columns are the camera's x, y and z
    axes in world coordinates (view = X @ R + T)."""
    pos = camera_position.reshape(-1, 3).to(torch.float32)
    up_t = torch.tensor(up, dtype=torch.float32).expand_as(pos)
    z = torch.nn.functional.normalize(-pos, eps=1e-5, dim=1)
    x = torch.nn.functional.normalize(torch.cross(up_t, z, dim=1), eps=1e-5, dim=1)
    y = torch.nn.functional.normalize(torch.cross(z, x, dim=1), eps=1e-5, dim=1)
    return torch.stack([x, y, z], dim=1).transpose(1, 2)


def uniform_cameras(distance: float = 12.0, elevation_deg: Optional[float] = None, n_cameras: int = 16,
                    camera_focal_length: float = 2.1875) -> Dict[str, Dict[str, torch.Tensor]]:
    """`get_uniform_camera` (cameras.py:117-139) as plain tensors: tag `U{i:03d}` -> {"R" (3, 3), "T" (3,), "focal_length" (2,),
    "principal_point" (2,), "position" (3,)}.  Camera i sits at L = (d sin(phi) cos(theta), d cos(phi), -d sin(phi) sin(theta)), phi
    (measured from +Y) cycling through 70, 55, 85, 40 degrees unless `elevation_deg` is given, theta = i / n * 360 degrees; R looks
    at the origin with up = +Y and T = -L @ R."""
    elevations = cycle([elevation_deg] if elevation_deg else [70, 55, 85, 40])
    cams = {}
    for i, elev in zip(range(n_cameras), elevations):
        theta, phi = math.radians(i / n_cameras * 360), math.radians(elev)
        L = torch.tensor([[distance * math.sin(phi) * math.cos(theta), distance * math.cos(phi),
                           -distance * math.sin(phi) * math.sin(theta)]], dtype=torch.float32)
        R = look_at_rotation(L)[0]
        cams[f"U{i:03d}"] = {"R": R, "T": (-L @ R)[0], "focal_length": torch.full((2,), float(camera_focal_length)),
                             "principal_point": torch.zeros(2), "position": L[0]}
    return cams


def project(points: torch.Tensor, camera: Dict[str, torch.Tensor]) -> torch.Tensor:
    """(N, 3) world points -> (N, 3) {x_ndc, y_ndc, view z}: the projection am_render_normals uses (PerspectiveCameras in NDC)."""
    v = points.to(torch.float32) @ camera["R"] + camera["T"]
    f, p = camera["focal_length"], camera["principal_point"]
    return torch.stack([f[0] * v[:, 0] / v[:, 2] + p[0], f[1] * v[:, 1] / v[:, 2] + p[1], v[:, 2]], dim=1)


# ---- image utilities (utils.py) ---------------------------------------------------------------------------------------------
def resample_list(items: list, target_length: int) -> list:
    """utils.py:16-36: nearest-neighbour resampling of a list to `target_length` entries."""
    if not items or target_length <= 0:
        return []
    n_in = len(items)
    if target_length == 1:
        return [items[0]]
    return [items[round(i * (n_in - 1) / (target_length - 1) + 1e-4)] for i in range(target_length)]


def make_image_grid(images: list, n_cols: int, image_size: Optional[int] = None):
    """utils.py:39-66: the images side by side (row-major), each resized to `image_size` square by PIL's default filter."""
    from PIL import Image
    if image_size is not None:
        images = [img.resize((image_size, image_size)) for img in images]
    n_rows = (len(images) + n_cols - 1) // n_cols
    w, h = images[0].size
    grid = Image.new("RGBA", (n_cols * w, n_rows * h), (0, 0, 0, 0))
    for idx, img in enumerate(images):
        grid.paste(img, ((idx % n_cols) * w, (idx // n_cols) * h))
    return grid


def _imageio():
    try:
        import imageio
        return imageio
    except ImportError:
        return None


def save_grid_video(frames: list, output_dir: str, name: str = "grid_normal", fps: int = FPS) -> str:
    """The grid frames as `<name>.mp4` through imageio (utils.py:69-86, the reference's file) when imageio is importable, else as a
    lossless animated PNG `<name>.png` (Pillow stores consecutive identical frames as one longer frame).  Both hold the frames' RGB.
    Returns the path written."""
    os.makedirs(output_dir, exist_ok=True)
    rgb = [f.convert("RGB") for f in frames]
    iio = _imageio()
    if iio is not None:
        path = os.path.join(output_dir, name + ".mp4")
        iio.mimsave(path, [np.array(f) for f in rgb], fps=fps)
        return path
    path = os.path.join(output_dir, name + ".png")
    rgb[0].save(path, format="PNG", save_all=True, append_images=rgb[1:], duration=1000.0 / fps, loop=0)
    return path


# ---- renderer / visualizer ----------------------------------------------------------------------------------------------------
def _camera_list(cameras) -> List[Dict[str, torch.Tensor]]:
    if isinstance(cameras, dict) and "R" in cameras:
        return [cameras]
    if isinstance(cameras, dict):
        return list(cameras.values())
    return list(cameras)


class HipRenderer:
    """The reference's `Renderer` (renderer.py:40-127) for the normal modality: hard raster at 2 x image_size, 2 x 2 average of the
    mask, nearest-sampled normal, white background."""

    def __init__(self, image_size: int = 256):
        self.image_size = int(image_size)

    def render_normals(self, vertices: torch.Tensor, faces: torch.Tensor, cameras, return_fragments: bool = False,
                       return_float: bool = False, device=None):
        """vertices (T, V, 3) (or (V, 3)), faces (F, 3), cameras: one camera dict, a list of them or a tag -> camera dict.
        Returns uint8 RGBA (T, C, S, S, 4) on the device; with `return_fragments` / `return_float` a dict that also holds
        "pix_to_face" / "bary" (2S x 2S) and "mask" / "normal"."""
        from . import ops
        device = torch.device(device) if device is not None else (vertices.device if vertices.is_cuda else torch.device("cuda"))
        v = torch.as_tensor(vertices)
        if v.dim() == 2:
            v = v[None]
        v = v.to(device=device, dtype=torch.float32).contiguous()
        out = ops.render_normals(v, torch.as_tensor(faces), _camera_list(cameras), self.image_size, fragments=return_fragments,
                                 floats=return_float)
        return out if (return_fragments or return_float) else out["rgba"]


def _stack_meshes(meshes, faces=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """A list of meshes (objects with .vertices / .faces on one topology, as the pipeline returns) or a (T, V, 3) stack with `faces`."""
    if faces is not None:
        return torch.as_tensor(np.asarray(meshes) if not isinstance(meshes, torch.Tensor) else meshes, dtype=torch.float32), \
            torch.as_tensor(np.asarray(faces)).to(torch.int64)
    meshes = list(meshes)
    if not meshes:
        raise ValueError("HipVisualizer.render: no meshes")
    f0 = np.asarray(meshes[0].faces)
    for m in meshes[1:]:
        if np.asarray(m.faces).shape != f0.shape or not np.array_equal(np.asarray(m.faces), f0):
            raise ValueError("HipVisualizer.render: the meshes do not share one topology")
    verts = np.stack([np.asarray(m.vertices, dtype=np.float32) for m in meshes])
    return torch.from_numpy(verts), torch.from_numpy(f0.astype(np.int64))


class HipVisualizer:
    """`ActionMeshVisualizer` (visualizer.py:57-152) on am_render_normals: same constructor, same `.render(meshes, device,
    output_dir, input_frames)`.  `bg_color` is kept for the signature: the normal modality composites on white, as the reference's
    `make_normal_image` does."""

    def __init__(self, image_size: int = 256, bg_color: Tuple[float, float, float] = (1.0, 1.0, 1.0),
                 cameras: Sequence[str] = VISUALIZER_CAMERAS):
        self.image_size = int(image_size)
        self.bg_color = bg_color
        self.renderer = HipRenderer(image_size)
        self.cameras = {k: v for k, v in uniform_cameras(distance=3.0).items() if k in cameras}

    def render_grid(self, meshes, device=None, input_frames: Optional[list] = None, faces=None) -> list:
        """The grid frames (PIL RGBA, one per mesh): the resampled input frame (if any), then one normal map per camera."""
        from PIL import Image
        verts, f = _stack_meshes(meshes, faces)
        n_frames = verts.shape[0]
        if input_frames is not None:
            input_frames = resample_list(list(input_frames), n_frames)
        rgba = self.renderer.render_normals(verts, f, self.cameras, device=device if device is not None else "cuda")
        rgba = rgba.cpu().numpy()
        n_cols = len(self.cameras) + (1 if input_frames is not None else 0)
        grid = []
        for t in range(n_frames):
            row = [input_frames[t]] if input_frames is not None else []
            row += [Image.fromarray(rgba[t, c], "RGBA") for c in range(rgba.shape[1])]
            grid.append(make_image_grid(row, n_cols, self.image_size))
        return grid

    def render(self, meshes, device=None, output_dir: str = ".", input_frames: Optional[list] = None, faces=None):
        """Render and write `grid_normal.mp4` (imageio) or `grid_normal.png` (animated PNG).  Returns ([path], grid frames)."""
        grid = self.render_grid(meshes, device=device, input_frames=input_frames, faces=faces)
        path = save_grid_video(grid, output_dir)
        logger.info("Saved render: %s", path)
        return [path], grid


# ---- the CLI hook -----------------------------------------------------------------------------------------------------------
_hook: Dict[str, Any] = {}


def pytorch3d_available() -> bool:
    """The reference script's own test (video_to_animated_mesh.py:26-37): can `pytorch3d` be imported?"""
    try:
        import pytorch3d  # noqa: F401
        return True
    except ImportError:
        return False


def install_hook() -> None:
    """Wrap `actionmesh.io.video_input.load_frames` and `actionmesh.io.mesh_io.save_deformation` (the names the reference scripts
    import at run time) so that the input, the meshes and the output directory of the run are kept for `render_captured`."""
    import actionmesh.io.mesh_io as MI
    import actionmesh.io.video_input as VI
    uninstall_hook()
    captured: Dict[str, Any] = {}
    orig_load, orig_save = VI.load_frames, MI.save_deformation

    def load_frames(*args, **kwargs):
        out = orig_load(*args, **kwargs)
        captured["input"] = out          # the pipeline replaces its .frames with the processed frames
        return out

    def save_deformation(meshes, path, *args, **kwargs):
        captured["meshes"] = meshes
        captured["output_dir"] = os.path.dirname(os.path.abspath(str(path)))
        return orig_save(meshes, path, *args, **kwargs)

    load_frames.__wrapped__, save_deformation.__wrapped__ = orig_load, orig_save
    VI.load_frames, MI.save_deformation = load_frames, save_deformation
    _hook.update(installed=True, modules=(VI, MI), saved=(orig_load, orig_save), captured=captured)


def uninstall_hook() -> None:
    if not _hook.get("installed"):
        return
    (VI, MI), (orig_load, orig_save) = _hook["modules"], _hook["saved"]
    VI.load_frames, MI.save_deformation = orig_load, orig_save
    _hook["installed"] = False


def hook_installed() -> bool:
    return bool(_hook.get("installed"))


def captured() -> Dict[str, Any]:
    return dict(_hook.get("captured", {}))


def render_captured(image_size: int = 256, device=None) -> Optional[List[str]]:
    """Render what the hooked run produced into its output directory (what the reference's visualizer call does); None when the
    run did not reach `save_deformation`."""
    cap = captured()
    if "meshes" not in cap:
        logger.warning("actionmesh_amd.render: the run saved no deformation; nothing to render")
        return None
    inp = cap.get("input")
    frames = getattr(inp, "frames", None) if inp is not None else None
    paths, _ = HipVisualizer(image_size=image_size).render(cap["meshes"], device=device, output_dir=cap["output_dir"],
                                                           input_frames=frames)
    return paths
