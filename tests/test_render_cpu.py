"""Preview rendering (INTEGRATION.md seam S6), the parts that need no GPU: the camera restatement of the reference's
`get_uniform_camera`, `resample_list`, the C-ABI struct and its argument checks, the grid / animated-PNG writer, and the CLI hook
that keeps what the reference script produced."""
import ctypes
import sys
import types

import numpy as np
import pytest
import torch

from actionmesh_amd import _lib
from actionmesh_amd import render as R


def test_uniform_cameras_restate_the_reference_layout():
    cams = R.uniform_cameras(distance=3.0)
    assert list(cams) == [f"U{i:03d}" for i in range(16)]
    s, c = np.sin(np.radians(70)), np.cos(np.radians(70))
    expect = {"U000": (3 * s, 3 * c, 0.0), "U004": (0.0, 3 * c, -3 * s), "U008": (-3 * s, 3 * c, 0.0)}
    for tag, pos in expect.items():
        cam = cams[tag]
        Rm, T = cam["R"].double(), cam["T"].double()
        centre = -T @ Rm.T                                   # view = X @ R + T = 0 at the camera centre
        assert np.allclose(centre.numpy(), pos, atol=1e-5), (tag, centre)
        assert np.allclose(cam["position"].numpy(), pos, atol=1e-5)
        assert abs(float(centre.norm()) - 3.0) < 1e-5
        assert abs(np.degrees(np.arccos(float(centre[1]) / 3.0)) - 70.0) < 1e-3      # 70 degrees from +Y
        assert np.allclose((Rm.T @ Rm).numpy(), np.eye(3), atol=1e-6) and abs(float(torch.det(Rm)) - 1.0) < 1e-6
        assert np.allclose(T.numpy(), (0.0, 0.0, 3.0), atol=1e-5)                    # the origin maps to view (0, 0, 3)
        o, up = R.project(torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.3, 0.0]]), cam)
        assert abs(float(o[0])) < 1e-6 and abs(float(o[1])) < 1e-6 and abs(float(o[2]) - 3.0) < 1e-5
        assert float(up[1]) > float(o[1]) + 0.1                                       # world +Y projects upwards
        assert torch.equal(cam["focal_length"], torch.full((2,), 2.1875)) and torch.equal(cam["principal_point"], torch.zeros(2))
    azimuths = [np.degrees(np.arctan2(-float(cams[t]["position"][2]), float(cams[t]["position"][0]))) % 360 for t in expect]
    assert np.allclose(azimuths, [0.0, 90.0, 180.0], atol=1e-4)
    elev = [np.degrees(np.arccos(float(cams[f"U{i:03d}"]["position"][1]) / 3.0)) for i in range(4)]
    assert np.allclose(elev, [70, 55, 85, 40], atol=1e-3)
    assert set(R.HipVisualizer().cameras) == {"U000", "U004", "U008"}


def test_resample_list_matches_the_reference_cases():
    assert R.resample_list(list(range(10)), 4) == [0, 3, 6, 9]
    assert R.resample_list(["a", "b", "c"], 5) == ["a", "b", "b", "c", "c"]      # round(0.5 + 1e-4) = 1
    assert R.resample_list(list(range(16)), 16) == list(range(16))
    assert R.resample_list(list(range(31)), 16) == [round(i * 30 / 15 + 1e-4) for i in range(16)]
    assert R.resample_list(["x", "y"], 1) == ["x"]
    assert R.resample_list([], 3) == [] and R.resample_list([1, 2], 0) == []


def test_render_argument_validation_without_gpu():
    """am_render_normals rejects bad counts, sizes and pointers before anything touches the device; the message comes from
    am_last_error.  (The face indices and the CSR are validated on the device: tests/test_render_gpu.py, test_guard_aux_gpu.py.)"""
    lib = _lib.lib()
    assert lib.am_render_normals(None, None, 0, None) != 0
    assert b"null" in lib.am_last_error()

    def args(**kw):
        a = _lib.AmRenderArgs()
        a.verts = a.faces = a.offsets = a.corners = a.out_flag = a.out_rgba = 16        # never dereferenced: the checks fail first
        a.n_frames, a.n_verts, a.n_faces, a.n_cameras, a.image_size = 1, 4, 2, 1, 8
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    big = 1 << 30
    for kw, msg in ((dict(faces=None), b"null pointer"), (dict(offsets=None), b"null pointer"), (dict(corners=None), b"null pointer"),
                    (dict(out_flag=None), b"null pointer"), (dict(verts=None), b"null pointer"), (dict(out_rgba=None), b"null pointer"),
                    (dict(n_faces=0), b"empty"), (dict(n_verts=0), b"empty"), (dict(n_frames=0), b"empty"),
                    (dict(n_cameras=17), b"cameras"), (dict(image_size=0), b"image size"),
                    (dict(n_frames=70000), b"grid"), (dict(n_frames=20000, n_verts=big // 1000), b"overflow")):
        a = args(**kw)
        assert lib.am_render_normals(ctypes.byref(a), None, 0, None) != 0, kw
        assert msg in lib.am_last_error(), (kw, lib.am_last_error())
    a = args()                                                   # valid sizes: only the missing workspace is left to refuse
    assert lib.am_render_normals(ctypes.byref(a), None, 0, None) != 0
    assert b"workspace" in lib.am_last_error()
    assert lib.am_render_workspace_bytes(1, 4, 2, 1, 8) > 0 and lib.am_render_workspace_bytes(0, 4, 2, 1, 8) == 0


def test_grid_and_animated_png_writer(tmp_path, monkeypatch):
    """make_image_grid lays the images out as the reference does; the animated PNG reads back as T frames of (C+1) S x S."""
    from PIL import Image
    monkeypatch.setattr(R, "_imageio", lambda: None)
    T, Cn, S = 5, 3, 32
    rng = np.random.default_rng(0)
    rgba = rng.integers(0, 256, size=(T, Cn, S, S, 4), dtype=np.uint8)
    rgba[..., 3] = 255
    inputs = [Image.fromarray(rng.integers(0, 256, size=(20, 28, 3), dtype=np.uint8), "RGB") for _ in range(T)]
    grid = [R.make_image_grid([inputs[t]] + [Image.fromarray(rgba[t, c], "RGBA") for c in range(Cn)], Cn + 1, S) for t in range(T)]
    g0 = np.array(grid[0])
    assert g0.shape == (S, (Cn + 1) * S, 4)
    assert np.array_equal(g0[:, :S, :3], np.array(inputs[0].resize((S, S)))) and (g0[:, :S, 3] == 255).all()
    for c in range(Cn):
        assert np.array_equal(g0[:, (c + 1) * S:(c + 2) * S], rgba[0, c])
    path = R.save_grid_video(grid, str(tmp_path / "out"))
    assert path.endswith("grid_normal.png")
    im = Image.open(path)
    assert im.n_frames == T and im.size == ((Cn + 1) * S, S)
    for t in range(T):
        im.seek(t)
        assert np.array_equal(np.array(im.convert("RGB")), np.array(grid[t].convert("RGB"))), t


def _stub(monkeypatch, name, **attrs):
    m = types.ModuleType(name)
    m.__path__ = []
    for k, v in attrs.items():
        setattr(m, k, v)
    monkeypatch.setitem(sys.modules, name, m)
    parent, _, child = name.rpartition(".")
    if parent:
        monkeypatch.setattr(sys.modules[parent], child, m, raising=False)
    return m


def test_install_render_wraps_and_uninstall_restores(monkeypatch, tmp_path):
    """install(render=True) wraps the two names the reference scripts import at run time (load_frames, save_deformation) and keeps
    what they return / receive; uninstall() puts the originals back."""
    from actionmesh_amd import dropin
    calls = []

    def load_frames(path, max_frames=None, stride=1):
        calls.append(("load", path))
        return types.SimpleNamespace(frames=["f0", "f1"])

    def save_deformation(meshes, path):
        calls.append(("save", path))
        return path + "_vertices.npy", path + "_faces.npy"

    _stub(monkeypatch, "actionmesh")
    _stub(monkeypatch, "actionmesh.pipeline", ActionMeshDenoiser=object, ActionMeshAutoencoder=object,
          load_config=lambda *a, **k: None)
    _stub(monkeypatch, "actionmesh.io")
    VI = _stub(monkeypatch, "actionmesh.io.video_input", load_frames=load_frames)
    MI = _stub(monkeypatch, "actionmesh.io.mesh_io", save_deformation=save_deformation)
    try:
        dropin.install(render=True)
        assert VI.load_frames is not load_frames and MI.save_deformation is not save_deformation and R.hook_installed()
        inp = VI.load_frames(path="clip.mp4", max_frames=31)
        out_dir = str(tmp_path / "run")
        assert MI.save_deformation(["m0", "m1"], path=f"{out_dir}/deformations") == (f"{out_dir}/deformations_vertices.npy",
                                                                                      f"{out_dir}/deformations_faces.npy")
        cap = R.captured()
        assert cap["input"] is inp and cap["meshes"] == ["m0", "m1"] and cap["output_dir"] == out_dir
        assert calls == [("load", "clip.mp4"), ("save", f"{out_dir}/deformations")]
        dropin.install(render=False)                 # re-install without the hook: the names are the originals again
        assert VI.load_frames is load_frames and MI.save_deformation is save_deformation
        dropin.install(render=True)
    finally:
        dropin.uninstall()
    assert VI.load_frames is load_frames and MI.save_deformation is save_deformation and not R.hook_installed()


def test_cli_render_option():
    from actionmesh_amd import cli
    ours, rest = cli.split_args(["--render", "off", "--", "--input", "a"])
    assert ours.render == "off" and rest == ["--input", "a"]
    assert cli.split_args(["--input", "a"])[0].render == "auto"
    with pytest.raises(SystemExit):
        cli.split_args(["--render", "pytorch3d"])
    assert R.pytorch3d_available() == (__import__("importlib").util.find_spec("pytorch3d") is not None)
