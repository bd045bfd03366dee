"""tests/golden/frames_raw/: the reference's example clips as RAW RGBA frames, and what its `ImagePreprocessor` makes of them.

TEST INFRASTRUCTURE ONLY.  Runs where the reference checkout is (the build container):

    python tools/make_golden_frames_raw.py [--reference DIR] [davis_camel panda kangaroo]

The frames are DATA (16 RGBA PNGs of 512 x 512 per clip, background already removed), stored losslessly as
`<clip>.<part>.npz` (key `rgba_u8`, (n, 512, 512, 4) uint8; consecutive parts in frame order, each part below the size limit of a
committed file - read them with `load_clip`).  `expected.json` records, per clip and for the shared and the independent crop, the
sizes (width, height: PIL's order) and a sha256 over the bytes of the RGB frames the reference's OWN
`ImagePreprocessor.process_images` returns (actionmesh/preprocessing/image_processor.py, imported unmodified by path, as
oracle/make_golden_frames.py does).  tests/test_image_preprocess_gpu.py holds the device path to them.
"""
import argparse
import glob
import hashlib
import io
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "frames_raw")
PART_LIMIT = 1000 * 1000        # bytes: below the 1 MiB limit of a committed file


def load_clip(clip: str, directory: str = OUT) -> np.ndarray:
    """(T, H, W, 4) uint8: the parts of a clip in order."""
    parts = sorted(glob.glob(os.path.join(directory, f"{clip}.*.npz")))
    if not parts:
        raise FileNotFoundError(f"no {clip}.*.npz under {directory}")
    return np.concatenate([np.load(p)["rgba_u8"] for p in parts], axis=0)


def frames_digest(images) -> dict:
    """sizes + sha256 of a list of RGB uint8 arrays (h, w, 3): each frame's bytes in order."""
    h = hashlib.sha256()
    for a in images:
        a = np.ascontiguousarray(a)
        assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3, (a.dtype, a.shape)
        h.update(a.tobytes())
    return {"sizes": [[int(a.shape[1]), int(a.shape[0])] for a in images], "sha256": h.hexdigest()}


def _compressed(arr: np.ndarray) -> bytes:
    buf = io.BytesIO()
    np.savez_compressed(buf, rgba_u8=arr)
    return buf.getvalue()


def write_parts(clip: str, rgba: np.ndarray) -> list:
    for old in glob.glob(os.path.join(OUT, f"{clip}.*.npz")):
        os.remove(old)
    names, start = [], 0
    while start < len(rgba):
        n = 1
        blob = _compressed(rgba[start: start + 1])
        while start + n < len(rgba):
            bigger = _compressed(rgba[start: start + n + 1])
            if len(bigger) > PART_LIMIT:
                break
            blob, n = bigger, n + 1
        assert len(blob) <= PART_LIMIT, (clip, start, len(blob))
        name = f"{clip}.{len(names):02d}.npz"
        with open(os.path.join(OUT, name), "wb") as fh:
            fh.write(blob)
        names.append(name)
        start += n
    return names


if __name__ == "__main__":
    import importlib.util
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("ACTIONMESH_ROOT", "/root/reference"))
    ap.add_argument("clips", nargs="*", default=["davis_camel", "panda", "kangaroo"])
    args = ap.parse_args()
    # the reference's module file, unmodified, loaded by path (its package __init__ imports modules that need cv2)
    spec = importlib.util.spec_from_file_location("ref_image_processor",
                                                  os.path.join(args.reference, "actionmesh", "preprocessing", "image_processor.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "expected.json")
    expected = json.load(open(path)) if os.path.exists(path) else {}
    for clip in args.clips:
        files = sorted(glob.glob(os.path.join(args.reference, "assets", "examples", clip, "*.png")))
        frames = [Image.open(f) for f in files]
        assert all(f.mode == "RGBA" for f in frames), [f.mode for f in frames]
        rgba = np.stack([np.ascontiguousarray(f) for f in frames])
        names = write_parts(clip, rgba)
        assert np.array_equal(load_clip(clip), rgba)
        entry = {"source": f"assets/examples/{clip} ({len(files)} frames)", "shape": list(rgba.shape), "parts": names}
        for key, independent in (("shared", False), ("independent", True)):
            out = mod.ImagePreprocessor(independent_cropping=independent).process_images(frames)      # reference
            entry[key] = frames_digest([np.asarray(im) for im in out])
        expected[clip] = entry
        print(clip, rgba.shape, names, entry["shared"]["sizes"][0], sorted(set(map(tuple, entry["independent"]["sizes"]))))
    with open(path, "w") as fh:
        json.dump(expected, fh, indent=1, sort_keys=True)
        fh.write("\n")
