"""`python -m actionmesh_amd.cli [--backend {hip,reference}] [--attn-dtype {bf16,fp8,fp8_fast}] [--stage1-fp32] [--stage2-hip [--stage2-cross-fp32] [--stage2-fp32]]
                                 [--render {auto,hip,off}] [--pointcloud {hip,off}] [--preprocess {hip,off}]
                                 [--mask-refine {hip,off}] [--isosurface {hip,hip-dual,off}] [--script NAME] [--reference-root DIR] -- <the reference CLI's own arguments>`

Runs the reference's UNMODIFIED command-line script (inference/video_to_animated_mesh.py:120-248, or
inference/video_and_3d_to_animated_mesh.py with `--script video_and_3d_to_animated_mesh`) with its own argument parser and
its own `--fast / --low_ram / --dtype / --stage_1_steps ...` flags, after `actionmesh_amd.install()` has put the MI355X
sampler and denoiser behind `ActionMeshPipeline` (actionmesh_amd/dropin.py): the preset the script derives from `--fast` /
`--low_ram` (lines 199-210) is served as its `_mi355x` overlay, and `ActionMeshDenoiser.from_pretrained` (pipeline.py:180)
builds a HipDenoiser.  `--backend reference` runs the same script untouched (`--backend {reference,hip}`).
The reference script keeps its code under `if __name__ == "__main__":`, so it is executed with runpy as `__main__`.
"""
from __future__ import annotations

import argparse
import os
import runpy
import sys
from typing import List, Optional, Tuple

SCRIPTS = ("video_to_animated_mesh", "video_and_3d_to_animated_mesh")


def find_script(name: str, reference_root: Optional[str]) -> str:
    roots = [reference_root, os.environ.get("ACTIONMESH_ROOT")]
    if not any(roots):
        import actionmesh          # the installed / checked-out reference: <root>/actionmesh/__init__.py
        roots.append(os.path.dirname(os.path.dirname(os.path.abspath(actionmesh.__file__))))
    for r in roots:
        if r:
            path = os.path.join(r, "inference", name + ".py")
            if os.path.isfile(path):
                return path
    raise FileNotFoundError(f"actionmesh_amd.cli: inference/{name}.py not found under {[r for r in roots if r]} "
                            "(pass --reference-root or set ACTIONMESH_ROOT)")


def split_args(argv: List[str]) -> Tuple[argparse.Namespace, List[str]]:
    """Our own options come first; everything else (after an optional `--`) is handed to the reference parser verbatim."""
    ap = argparse.ArgumentParser(prog="python -m actionmesh_amd.cli", add_help=False,
                                 description="Run the reference ActionMesh CLI on the MI355X backend (or untouched).")
    ap.add_argument("--backend", choices=["hip", "reference"], default="hip")
    ap.add_argument("--attn-dtype", choices=["bf16", "fp8", "fp8_fast"], default="bf16",
                    help="inflated self-attention arithmetic: bf16 (default), e4m3 MFMA (fp8), or its exponent-field form (fp8_fast)")
    ap.add_argument("--stage2-hip", action="store_true", help="also decode Stage II on the HIP kernels (HipAutoencoder)")
    ap.add_argument("--stage2-cross-fp32", action="store_true",
                    help="with --stage2-hip: Stage II's query side and cross-attention block in exact fp32, as the reference runs them")
    ap.add_argument("--stage2-fp32", action="store_true",
                    help="with --stage2-hip: all of Stage II in exact fp32 (HipAutoencoder(exact_fp32=True)): the reference's fp32 arithmetic on "
                         "the device, the ground truth for a 16-bit run of the same checkpoint - many times slower; implies --stage2-cross-fp32")
    ap.add_argument("--stage1-fp32", action="store_true",
                    help="with --backend hip: Stage I in exact fp32 (HipDenoiser(dtype='float32')): the reference's fp32 arithmetic on the "
                         "device, the ground truth for a 16-bit or fp8 run of the same checkpoint - many times slower; needs --attn-dtype bf16")
    ap.add_argument("--render", choices=["auto", "hip", "off"], default="auto",
                    help="with --backend hip: the preview video grid_normal.* on HIP after the script: auto (default) = only when pytorch3d is not "
                         "importable, so the reference's own video is not rendered twice; hip = always; off = never")
    ap.add_argument("--pointcloud", choices=["hip", "off"], default="off",
                    help="with --backend hip: hip = give actionmesh.external.triposg the sample_pc / masked_gather it lacks without pytorch3d, "
                         "over the HIP farthest-point sampling (the {video+3D} script's anchor latent); off (default) = leave it alone")
    ap.add_argument("--preprocess", choices=["hip", "off"], default="off",
                    help="with --backend hip: hip = crop / pad the frames and resize / crop / normalise them for DINOv2 on the device, bit-identical "
                         "to the reference's CPU code (HipImagePreprocessor, HipImageEncoder(preprocess='hip')); off (default) = leave both alone")
    ap.add_argument("--mask-refine", choices=["hip", "off"], default="off",
                    help="with --backend hip: hip = the background remover's refine_mask (Otsu threshold, connected components, removal of "
                         "the small ones) on the HIP labelling kernels, without cv2 / skimage arithmetic; off (default) = leave it alone")
    ap.add_argument("--isosurface", choices=["hip", "hip-dual", "off"], default="off",
                    help="with --backend hip: hip = TripoSG's hierarchical_extract_geometry behind the Stage-0 VAE on the HIP marching "
                         "tetrahedra, without the diso wheel; hip-dual = the same on the HIP dual marching cubes (about a third of the "
                         "triangles); off (default) = leave it alone")
    ap.add_argument("--script", choices=SCRIPTS, default=SCRIPTS[0])
    ap.add_argument("--reference-root", default=None)
    ap.add_argument("--amd-help", action="store_true", help="this wrapper's options (plain --help shows the reference CLI's)")
    ours, rest = ap.parse_known_args(argv)
    if rest and rest[0] == "--":
        rest = rest[1:]
    if ours.amd_help:
        ap.print_help()
        raise SystemExit(0)
    if ours.stage2_cross_fp32 and not ours.stage2_hip:
        ap.error("--stage2-cross-fp32 needs --stage2-hip")
    if ours.stage2_fp32 and not ours.stage2_hip:
        ap.error("--stage2-fp32 needs --stage2-hip")
    if ours.stage1_fp32 and (ours.backend != "hip" or ours.attn_dtype != "bf16"):
        ap.error("--stage1-fp32 needs --backend hip and --attn-dtype bf16")
    return ours, rest


def main(argv: Optional[List[str]] = None) -> None:
    ours, rest = split_args(list(sys.argv[1:] if argv is None else argv))
    if ours.reference_root:
        sys.path.insert(0, ours.reference_root)
    script = find_script(ours.script, ours.reference_root)
    render = False
    if ours.backend == "hip":
        from . import dropin
        from . import render as R
        render = ours.render == "hip" or (ours.render == "auto" and not R.pytorch3d_available())
        dropin.install(attn_dtype=ours.attn_dtype, stage2=ours.stage2_hip, stage2_cross_fp32=ours.stage2_cross_fp32, render=render,
                       pointcloud=ours.pointcloud == "hip")
        if ours.stage1_fp32:
            dropin.install_stage1_fp32()
        if ours.stage2_fp32:
            dropin.install_stage2_fp32()
        if ours.preprocess == "hip":
            dropin.install_preprocess()
        if ours.mask_refine == "hip":
            dropin.install_mask_refine()
        if ours.isosurface != "off":
            dropin.install_isosurface(method="dual" if ours.isosurface == "hip-dual" else "tetrahedra")
    old_argv = sys.argv
    sys.argv = [script] + rest
    try:
        runpy.run_path(script, run_name="__main__")
    finally:
        sys.argv = old_argv
    if render:           # the preview video the reference renders only with PyTorch3D (seam S6), into the script's output directory
        R.render_captured()


if __name__ == "__main__":
    main()
