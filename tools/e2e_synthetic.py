#!/usr/bin/env python
"""GPU part of the video -> 4D pipeline, end to end on synthetic data, one MI355X:

    frames (T x 3 x 224 x 224)  --HipImageEncoder (DINOv2 ViT-L/14)-->  context (T, 257, 1024)
    anchor latent + context     --generate_3d_latents (Stage I: AR windows of 16 frames, flow matching, CFG)-->  latents
    latents + anchor vertices   --generate_vertex_animation (Stage II: ActionMeshAutoencoder per window)-->  vertices per frame

at the shipped shapes (Stage I: N = 2048 tokens, width 2048, 16 heads, 21 layers; Stage II: width 1024, 16 + 1 blocks) with
random-init weights.  The anchor is a torus mesh; its per-window vertex features (positions + angle-weighted vertex normals) are
`actionmesh_amd.VertexFeatures` on the device (`--features analytic`: the earlier stand-in, normalised positions, no kernel).  What
stays on the reference's CPU path (and is not timed here): background removal, TripoSG Stage 0.  Prints one JSON line (secondary metric:
BASELINE.json's "end-to-end video->4D wall-clock" restricted to the stages this repository implements).

    python tools/e2e_synthetic.py [--frames 16] [--steps 30] [--vertices 50000] [--tiny]
    python tools/e2e_synthetic.py --exact-fp32 [--steps 3]      the same chain twice on the same inputs and seeds - the default models, and
                                                  encoder fp32 -> Stage I fp32 -> Stage II fp32 (exact_fp32=True) - and the default run's vertex
                                                  error against the exact one, in the normalised mesh's units; a short step count, stated in the record
    python tools/e2e_synthetic.py --config 1      BASELINE.json configs[1]: the 16 davis_camel frames (tests/golden/frames/, preprocessed by the
                                                  reference's own ImagePreprocessor + BitImageProcessor geometry), 50-step scheduler, bf16
    python tools/e2e_synthetic.py --config 3      configs[3]: the panda clip; in the reference this path (pipeline_with_3d) differs from configs[1]
                                                  ONLY in where the anchor latent / mesh come from (a given panda.glb through the TripoSG VAE
                                                  encoder instead of TripoSG's image-to-3D sampler) - both are Stage 0, on the reference path;
                                                  here the anchor latent is seeded noise in both; the given mesh is a deliberately DIRTY torus
                                                  (duplicated seam vertices, degenerate and duplicate faces, GLB units) that goes through
                                                  merge_and_clean_mesh -> normalize_mesh -> sample_surface(16384) in front of Stage II and
                                                  through denormalize_mesh + expand_to_original behind it (pipeline_with_3d.py:92-104, 229-238)
    python tools/e2e_synthetic.py --config 3 --face-decimation N --field-grid G     opt-in: the mesh itself comes from an analytic torus field
                                                  on G^3 points, extracted on the device (extract_isosurface, seam S11), then as below
    python tools/e2e_synthetic.py --config 3 --face-decimation N      opt-in: the dirty torus goes through the reference's Stage-0 post-processing
                                                  instead - process_mesh(face_decimation=N, decimation="hip"): clean-up, then the quadric decimation
                                                  on the device (actionmesh_amd/mesh_decimate.py; MeshPostprocessor.process_mesh, pipeline.py:418) -
                                                  and Stage II animates the decimated mesh; a decimated mesh has no map back to the given one, so
                                                  the animation stays on it
    python tools/e2e_synthetic.py --config 3 --face-decimation N --decimate-borders collapse     the same with process_mesh(decimate_borders="collapse"):
                                                  border collapses permitted; the torus is closed, so the mesh is the same bits
Both are PLUMBING records on random-init weights (no checkpoint is reachable offline): not BASELINE's end-to-end metric.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rand_like_spec(shapes, g):
    sd = {}
    for name, shape in shapes.items():
        if name.endswith(".weight") and len(shape) >= 2:
            fan = 1
            for s in shape[1:]:
                fan *= s
            sd[name] = torch.randn(shape, generator=g) / fan ** 0.5
        elif name.endswith(".weight") or name.endswith("lambda1"):
            sd[name] = torch.ones(shape)
        elif name.startswith("embeddings.") and not name.endswith(".bias"):
            sd[name] = 0.5 * torch.randn(shape, generator=g)
        else:
            sd[name] = torch.zeros(shape)
    return sd


def build(tiny: bool, dev, exact: bool = False):
    """The three models on random-init weights; `exact`: each in its exact-fp32 mode, from the same weights."""
    from bench import random_state_dict
    from actionmesh_amd import ClassifierFreeGuidance, HipAutoencoder, HipDenoiser, HipImageEncoder, HipSchedulerFlow
    from actionmesh_amd import image_encoder as IE
    g = torch.Generator().manual_seed(0)
    if tiny:
        dino = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, image_size=56)
        den = dict(in_channels=64, num_layers=3, num_attention_heads=2, width=256, mlp_ratio=4.0, cross_attention_dim=128,
                   inflated_layers=[0, 1, 2])
        ae = dict(width=256, num_layers=2, num_attention_heads=2, latent_channels=64)
        n_tokens, window, side = 40, 4, 56
    else:
        dino = {}
        den = dict(in_channels=64, num_layers=21, num_attention_heads=16, width=2048, mlp_ratio=4.0, cross_attention_dim=1024,
                   inflated_layers=list(range(21)))
        ae = dict(width=1024, num_layers=16, num_attention_heads=8, latent_channels=64)
        n_tokens, window, side = 2048, 16, 224
    enc = HipImageEncoder(config=dino, state_dict=rand_like_spec(IE.state_dict_shapes(dict(IE._CFG_DEFAULTS, **dino)), g),
                          **(dict(dtype="float32") if exact else {})).to(dev)
    denoiser = HipDenoiser(num_tokens_nominal=n_tokens, temporal_context_size=window, **den, **(dict(dtype="float32") if exact else {}))
    denoiser.load_state_dict(random_state_dict(den, seed=0))
    denoiser.to(dev).eval()
    from oracle.autoencoder_oracle import AEConfig, state_dict_spec      # parameter names / shapes only
    vae = HipAutoencoder(temporal_context_size=window, **ae, exact_fp32=exact)
    vae.load_state_dict(rand_like_spec(dict(state_dict_spec(AEConfig(**ae))), g))
    vae.to(dev)
    return enc, denoiser, vae, HipSchedulerFlow, ClassifierFreeGuidance, n_tokens, window, side


def torus_mesh(vertices: int):
    """A torus of exactly `vertices` vertices (rows x cols, rows the largest divisor of `vertices` up to its square root) inside the
    0.8 cube: fp64 (V, 3), int64 (2 V, 3), numpy; and cols."""
    import numpy as np
    rows = max((d for d in range(3, int(vertices ** 0.5) + 1) if vertices % d == 0), default=0)
    if rows == 0:
        raise ValueError(f"--vertices {vertices} must be rows x cols with both at least 3")
    cols = vertices // rows
    a, b = np.meshgrid(2 * np.pi * np.arange(rows) / rows, 2 * np.pi * np.arange(cols) / cols, indexing="ij")
    v = np.stack(((0.55 + 0.25 * np.cos(a)) * np.cos(b), (0.55 + 0.25 * np.cos(a)) * np.sin(b), 0.25 * np.sin(a)), -1).reshape(-1, 3)
    i, j = (x.reshape(-1) for x in np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij"))
    p00, p01 = i * cols + j, i * cols + (j + 1) % cols
    p10, p11 = (i + 1) % rows * cols + j, (i + 1) % rows * cols + (j + 1) % cols
    return v, np.concatenate((np.stack((p00, p01, p11), 1), np.stack((p00, p11, p10), 1))).astype(np.int64), cols


def dirty_mesh(v, f, cols: int, seed: int = 2):
    """What a GLB loader hands over: the vertices of the seam column duplicated (half of them moved by up to 2e-9) with the faces
    on one side of the seam naming the copies, eight faces with a repeated index and eight repeated faces with reversed winding
    scattered through the face array, everything in model units (x 3, shifted)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    seam = np.arange(0, len(v), cols)                                   # column 0 of every row
    moved = v[seam] + rng.uniform(-2e-9, 2e-9, (len(seam), 3)) * (rng.random((len(seam), 1)) < 0.5)
    v2 = np.concatenate((v, moved)) * 3.0 + (5.0, -2.0, 1.0)
    same_key = (np.round(v2[len(v):] * 1e8) == np.round(v2[seam] * 1e8)).all(1, keepdims=True)
    v2[len(v):] = np.where(same_key, v2[len(v):], v2[seam])             # a copy the 1e-8 grid would separate stays exact
    copy_of = np.arange(len(v))
    copy_of[seam] = len(v) + np.arange(len(seam))
    f2 = f.copy()
    wrap = (f % cols == cols - 1).any(1)                                # faces that reach the seam from the last column
    f2[wrap] = np.where(np.isin(f[wrap], seam), copy_of[f[wrap]], f[wrap])
    extra = [(a, b, a) for a, b in rng.integers(0, len(v2), (8, 2)) if a != b]
    extra += [tuple(f2[k][::-1]) for k in rng.integers(0, len(f2), 8)]
    for face in extra:
        f2 = np.insert(f2, rng.integers(len(f2) // 2, len(f2) + 1), face, axis=0)      # behind the face it repeats, or anywhere
    return v2, f2


def run(frames: int, steps: int, vertices: int, tiny: bool, dev, seed: int = 44, clip: str = None, label: str = None,
        raw_frames: bool = False, features: str = "hip", mesh_prep: bool = False, face_decimation: int = 0, field_grid: int = 0,
        iso_method: str = "tetrahedra", decimate_borders: str = "fixed"):
    from actionmesh_amd import LatentBank, generate_3d_latents, generate_vertex_animation
    from actionmesh_amd import mesh_prep as MP
    t_build = time.perf_counter()
    enc, denoiser, vae, Sched, CFG, n_tokens, window, side = build(tiny, dev)
    torch.cuda.synchronize(dev)
    t_build = time.perf_counter() - t_build
    g = torch.Generator().manual_seed(1)
    t_pre = None
    if clip and raw_frames:        # from the raw RGBA frames (tests/golden/frames_raw): crop, pad, resize, normalise on the device
        import numpy as np
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from make_golden_frames_raw import load_clip
        from actionmesh_amd import image_preprocess as IP
        settings = IP.processor_settings({"size": {"shortest_edge": 256}, "crop_size": {"height": side, "width": side}, "resample": 3,
                                          "image_mean": [0.485, 0.456, 0.406], "image_std": [0.229, 0.224, 0.225]})
        raw = load_clip(clip)
        assert raw.shape[0] >= frames, (raw.shape, frames)
        IP.frames_to_pixel_values(torch.from_numpy(raw[:1]).to(dev), settings)          # the library's first call, outside the stage
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        pixels = IP.frames_to_pixel_values(torch.from_numpy(raw[:frames]).to(dev), settings)   # the upload is part of the stage
        torch.cuda.synchronize(dev)
        t_pre = time.perf_counter() - t0
        if frames == raw.shape[0] and side == 224 and os.path.exists(os.path.join(ROOT, "tests", "golden", "frames", f"{clip}_16x224.npz")):
            from oracle.make_golden_frames import frames_to_pixels
            rgb = np.load(os.path.join(ROOT, "tests", "golden", "frames", f"{clip}_16x224.npz"))["rgb_u8"]
            assert float((pixels.cpu() - frames_to_pixels(rgb)).abs().max()) < 1e-6      # the frames the committed fixture holds
    elif clip:           # a real clip as the context encoder receives it (oracle/make_golden_frames.py)
        import numpy as np
        from oracle.make_golden_frames import frames_to_pixels          # the rescale + normalise half of BitImageProcessor (data handling only)
        rgb = np.load(os.path.join(ROOT, "tests", "golden", "frames", f"{clip}_16x224.npz"))["rgb_u8"]
        assert rgb.shape[0] >= frames and rgb.shape[1] == side, (rgb.shape, frames, side)
        pixels = frames_to_pixels(rgb[:frames]).to(dev)
    else:
        pixels = torch.randn((frames, 3, side, side), generator=g).to(dev)
    timesteps = torch.arange(frames, dtype=torch.float32)
    anchor_latent = torch.randn((1, n_tokens, 64), generator=g).to(dev)
    clean_v, clean_f, cols = torus_mesh(vertices)
    t_prep = t_iso = None
    if mesh_prep:          # the {video+3D} front end: dirty mesh -> clean-up -> normalise -> surface samples, all on the device
        if field_grid:     # Stage 0's last step first: the mesh is extracted on the device from an analytic torus field (seam S11)
            from actionmesh_amd import isosurface as ISO
            ax = torch.linspace(-1.0, 1.0, field_grid, dtype=torch.float64, device=dev)
            gx, gy, gz = torch.meshgrid(ax, ax, ax, indexing="ij")
            field = (0.25 - (((gx * gx + gy * gy).sqrt() - 0.6) ** 2 + gz * gz).sqrt()).float()
            ISO.extract_isosurface(field[:9, :9, :9], bounds=1.0, method=iso_method)       # the library's first call, outside the stage
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            raw_v, raw_f = ISO.extract_isosurface(field, bounds=1.0, method=iso_method)
            torch.cuda.synchronize(dev)
            t_iso = time.perf_counter() - t0
            assert raw_f.shape[0] > face_decimation, (raw_f.shape, face_decimation)
            raw_v = raw_v.double() * 3.0 + torch.tensor((5.0, -2.0, 1.0), dtype=torch.float64, device=dev)      # model units
        else:
            raw_v, raw_f = (torch.from_numpy(x).to(dev) for x in dirty_mesh(clean_v, clean_f, cols))
        warm_v, warm_f, _, _ = MP.merge_and_clean_mesh(raw_v, raw_f)     # the library's first calls, outside the stage
        MP.sample_surface(MP.normalize_mesh(warm_v)[0], warm_f, 16, seed=0)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        if face_decimation:    # the reference's Stage-0 post-processing: clean-up, then the quadric decimation, both on the device
            anchor_v, faces = MP.process_mesh(raw_v, raw_f, face_decimation=face_decimation, decimation="hip",
                                              decimate_borders=decimate_borders)
            merge_map = pre_faces = None
        else:
            anchor_v, faces, merge_map, pre_faces = MP.merge_and_clean_mesh(raw_v, raw_f)
        anchor_v, norm_params = MP.normalize_mesh(anchor_v)
        cloud = MP.sample_surface(anchor_v, faces, 16384, seed=0, with_normals=True, dtype=torch.bfloat16)   # the VAE encoder's input
        torch.cuda.synchronize(dev)
        t_prep = time.perf_counter() - t0
        if face_decimation:
            assert faces.shape[0] in (face_decimation, face_decimation - 1) and int(faces.max()) == anchor_v.shape[0] - 1, (anchor_v.shape, faces.shape)
            vertices = anchor_v.shape[0]
        else:
            assert anchor_v.shape[0] == vertices and faces.shape[0] == len(clean_f) and raw_v.shape[0] > vertices, (anchor_v.shape, faces.shape)
        assert cloud.shape == (1, 16384, 6) and bool(torch.isfinite(cloud.float()).all())
        pts = anchor_v.float()
    else:
        pts, faces = torch.from_numpy(clean_v).float().to(dev), torch.from_numpy(clean_f).to(dev)
    if features == "hip":
        features = MP.VertexFeatures(faces)                            # positions | angle-weighted vertex normals, per window
    else:                                                              # the earlier stand-in: the normalised position as a normal
        features = lambda v: torch.cat([v, torch.nn.functional.normalize(v, dim=-1)], dim=-1)
    sched, cfg = Sched(num_inference_steps=steps, shift=3.0, is_additive=True), CFG(True, [[0, 1], [1, 1]], [7.5])
    slide = window - 1

    def stage(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return out, time.perf_counter() - t0

    context, t_enc = stage(lambda: enc.encode_pixels(pixels))
    bank = LatentBank(empty_dims=(n_tokens, 64), device=str(dev))
    bank.update(timesteps[:1], anchor_latent)
    bank, t_s1 = stage(lambda: generate_3d_latents(denoiser, sched, cfg, timesteps, context, bank, 0, window, slide,
                                                   (n_tokens, 64), seed=seed, device=dev))
    vbank = LatentBank(empty_dims=(vertices, 3), device=str(dev))
    vbank.update(timesteps[:1], pts[None])
    vbank, t_s2 = stage(lambda: generate_vertex_animation(vae, bank, vbank, features, 0, window, slide, device=dev))
    verts, ts = vbank.get_ordered()
    assert ts.tolist() == timesteps.tolist() and verts.shape == (frames, vertices, 3)
    assert bool(torch.isfinite(verts).all()) and float(verts.abs().max()) <= 1.0
    lat, _ = bank.get_ordered()
    assert bool(torch.isfinite(lat).all())
    # output files (N4): per-frame GLBs, the deformation arrays, the animated morph-target GLB, the preview video; and the ActionBench Chamfer metrics
    # of the animation against itself shifted by one frame (a number that must be > 0 and finite: the metric path end to end)
    import shutil
    import tempfile
    from actionmesh_amd import actionbench, create_animated_glb, save_deformation, save_meshes
    t_back = None
    if mesh_prep and merge_map is not None:          # back to the given mesh: model units, the original (pre-merge) topology
        (verts_out, t_back) = stage(lambda: MP.expand_to_original(MP.denormalize_mesh(verts.double(), norm_params), merge_map).float())
        assert verts_out.shape == (frames, raw_v.shape[0], 3) and float((verts_out[0] - raw_v).abs().max()) < 1e-5
        verts, faces = verts_out, pre_faces
    faces = faces.cpu()
    out_dir = tempfile.mkdtemp(prefix="am_e2e_")
    t0 = time.perf_counter()
    save_meshes(verts, faces, os.path.join(out_dir, "meshes"))
    vp, fp = save_deformation(verts, faces, os.path.join(out_dir, "deformations"))
    create_animated_glb(vertices_npy=str(vp), faces_npy=str(fp), output_glb=os.path.join(out_dir, "animated_mesh.glb"), fps=8)
    t_out = time.perf_counter() - t0
    # the preview video (grid_normal.*: three normal-map views per frame, the reference's visualizer call) on am_render_normals
    from actionmesh_amd import HipVisualizer
    t0 = time.perf_counter()
    HipVisualizer(image_size=256).render(verts, device=dev, output_dir=out_dir, input_frames=None, faces=faces)
    t_preview = time.perf_counter() - t0
    out_bytes = sum(os.path.getsize(os.path.join(r, f_)) for r, _, fs in os.walk(out_dir) for f_ in fs)
    shutil.rmtree(out_dir)
    (cd, cdm), t_metric = stage(lambda: (actionbench.compute_chamfer_score(verts[1], verts[0], device=dev),
                                         actionbench.compute_motion_chamfer_score(verts[1:], verts[:-1], device=dev)))
    assert cd > 0 and cdm > 0 and cd == cd and cdm == cdm
    n_win = len(__import__("actionmesh_amd").chunk_from(0, frames, window, slide))
    return {"metric": "video->4D wall-clock, GPU stages (context encoder + Stage I + Stage II)", "value": round(t_enc + t_s1 + t_s2, 3),
            "unit": "s", "higher_is_better": False, "n_gpus": 1, "dtype": "bf16", "data": "synthetic",
            "seconds": {"context_encoder": round(t_enc, 4), "stage_I": round(t_s1, 3), "stage_II": round(t_s2, 3),
                        "model_build_and_upload": round(t_build, 1),
                        **({"preprocess_s": round(t_pre, 4)} if t_pre is not None else {}),
                        **({"mesh_prep": round(t_prep, 4)} if mesh_prep else {}),
                        **({"isosurface": round(t_iso, 4)} if t_iso is not None else {}),
                        **({"mesh_back_to_original": round(t_back, 4)} if t_back is not None else {}),
                        "output_files_host_side": round(t_out, 3), "chamfer_metrics": round(t_metric, 4)},
            "preview_video_s": round(t_preview, 3),          # grid_normal.* (HipVisualizer), written into the output files above
            "output_files_mb": round(out_bytes / 1e6, 1),
            "config": {"workload": f"{frames} frames, {n_win} AR window(s) of {window}, {steps} denoise steps, N={n_tokens} tokens, "
                                   f"{vertices} vertices, {'tiny' if tiny else 'shipped'} model shapes, random-init weights"
                                   + (f", frames = the reference's {clip} clip" if clip else ", random frames")
                                   + (f", mesh extracted from a {field_grid}^3 torus field on the device ({iso_method})" if field_grid else "")
                                   + (f", decimated to {faces.shape[0]} faces on the device" if face_decimation else "")},
            **({"baseline_config": label} if label else {}),
            "context_rms": round(float(context.float().pow(2).mean().sqrt()), 4), "latents_rms": round(float(lat[1:].float().pow(2).mean().sqrt()), 4)}


def run_exact_fp32(frames: int, steps: int, vertices: int, tiny: bool, dev, seed: int = 44):
    """How far the default pipeline's vertices are from the same pipeline in exact arithmetic: the chain context encoder -> Stage I
    windows -> Stage II windows twice on the same pixels, anchor latent, anchor mesh and seeds (the noise is drawn on the device from
    the window's seed in both) - the default models, then every stage in its exact-fp32 mode - and the vertex error of the first
    against the second, in the units of the normalised mesh (the torus fills the 0.8 cube)."""
    from actionmesh_amd import LatentBank, generate_3d_latents, generate_vertex_animation
    from actionmesh_amd import mesh_prep as MP
    clean_v, clean_f, _ = torus_mesh(vertices)
    out, seconds = {}, {}
    for mode in ("default", "exact_fp32"):
        enc, denoiser, vae, Sched, CFG, n_tokens, window, side = build(tiny, dev, exact=mode == "exact_fp32")
        g = torch.Generator().manual_seed(1)
        pixels = torch.randn((frames, 3, side, side), generator=g).to(dev)
        timesteps = torch.arange(frames, dtype=torch.float32)
        anchor_latent = torch.randn((1, n_tokens, 64), generator=g).to(dev)
        pts, faces = torch.from_numpy(clean_v).float().to(dev), torch.from_numpy(clean_f).to(dev)
        features = MP.VertexFeatures(faces)
        sched, cfg = Sched(num_inference_steps=steps, shift=3.0, is_additive=True), CFG(True, [[0, 1], [1, 1]], [7.5])
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        context = enc.encode_pixels(pixels)
        bank = LatentBank(empty_dims=(n_tokens, 64), device=str(dev))
        bank.update(timesteps[:1], anchor_latent)
        generate_3d_latents(denoiser, sched, cfg, timesteps, context, bank, 0, window, window - 1, (n_tokens, 64), seed=seed, device=dev)
        vbank = LatentBank(empty_dims=(vertices, 3), device=str(dev))
        vbank.update(timesteps[:1], pts[None])
        generate_vertex_animation(vae, bank, vbank, features, 0, window, window - 1, device=dev)
        torch.cuda.synchronize(dev)
        seconds[mode] = round(time.perf_counter() - t0, 3)
        verts, ts = vbank.get_ordered()
        assert ts.tolist() == timesteps.tolist() and bool(torch.isfinite(verts).all())
        out[mode] = (verts.double().cpu(), bank.get_ordered()[0].double().cpu(), context.double().cpu())
        denoiser.cpu(); vae.to("cpu")
        del enc, denoiser, vae, bank, vbank, context
        torch.cuda.empty_cache()
    (v, lat, ctx), (v32, lat32, ctx32) = out["default"], out["exact_fp32"]
    assert torch.equal(v[0], v32[0])                                     # the anchor mesh, kept by both
    dist = (v[1:] - v32[1:]).norm(dim=-1)                                # (frames - 1, V): Euclidean, per vertex and frame
    rel = lambda a, b: float((a - b).norm() / b.norm())
    return {"metric": "default (bf16) pipeline's vertices against the exact-fp32 pipeline, same inputs and seeds", "value": rel(v[1:], v32[1:]),
            "unit": "rel-L2", "higher_is_better": False, "n_gpus": 1, "data": "synthetic", "denoise_steps": steps,
            "vertex_error": {"rel_l2": rel(v[1:], v32[1:]), "mean_euclidean": float(dist.mean()), "max_euclidean": float(dist.max()),
                             "units": "normalised mesh (torus inside the 0.8 cube)",
                             "per_frame_max_euclidean": [float(x) for x in dist.max(dim=1).values]},
            "context_rel_l2": rel(ctx, ctx32), "latents_rel_l2": rel(lat[1:], lat32[1:]),
            "seconds_gpu_stages": seconds,
            "config": {"workload": f"{frames} frames, AR windows of {window}, {steps} denoise steps (short on purpose: the exact Stage I is many "
                                   f"times slower), N={n_tokens} tokens, {vertices} vertices, {'tiny' if tiny else 'shipped'} model shapes, "
                                   "random-init weights, random frames"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--steps", type=int, default=None, help="denoise steps per window (default 30; 3 with --exact-fp32)")
    ap.add_argument("--exact-fp32", action="store_true",
                    help="run the chain in the default modes and in exact fp32 (encoder, Stage I, Stage II) on the same inputs and seeds, and "
                         "report the default run's vertex error against the exact one")
    ap.add_argument("--vertices", type=int, default=50000)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--clip", default=None, choices=["davis_camel", "panda"], help="frames of a reference example clip (tests/golden/frames/) instead of noise")
    ap.add_argument("--raw-frames", action="store_true",
                    help="with --clip: start from the raw RGBA frames (tests/golden/frames_raw/) and preprocess them on the device; adds preprocess_s")
    ap.add_argument("--features", default="hip", choices=["hip", "analytic"],
                    help="Stage II's vertex features: VertexFeatures on the device (default), or the earlier stand-in (normalised positions)")
    ap.add_argument("--mesh-prep", action="store_true", help="start from a dirty mesh and run the {video+3D} mesh glue around Stage II (implied by --config 3)")
    ap.add_argument("--face-decimation", type=int, default=0,
                    help="with --mesh-prep / --config 3: decimate the cleaned mesh to this many faces on the device (process_mesh(decimation='hip'))")
    ap.add_argument("--decimate-borders", default="fixed", choices=["fixed", "collapse"],
                    help="with --face-decimation: process_mesh(decimate_borders=...) - 'collapse' lets an open mesh reach the target too; "
                         "on the closed meshes of this tool both give the same bits")
    ap.add_argument("--field-grid", type=int, default=0, metavar="N",
                    help="with --face-decimation: start from an analytic torus field on N^3 points instead of a prepared mesh - "
                         "extract_isosurface on the device, then the clean-up and the decimation (adds seconds.isosurface)")
    ap.add_argument("--iso-method", default="tetrahedra", choices=["tetrahedra", "dual"],
                    help="with --field-grid: the extraction - marching tetrahedra (default) or dual marching cubes (about a third of the "
                         "triangles in front of the decimation)")
    ap.add_argument("--config", type=int, default=None, choices=[1, 3], help="BASELINE.json configs[1] / configs[3] as a plumbing record (see the module docstring)")
    a = ap.parse_args()
    if a.steps is None:
        a.steps = 3 if a.exact_fp32 else 30
    if a.exact_fp32 and (a.clip or a.config or a.mesh_prep or a.face_decimation):
        ap.error("--exact-fp32 runs the plain chain on random frames: no --clip, --config, --mesh-prep or --face-decimation")
    if a.raw_frames and not (a.clip or a.config):
        ap.error("--raw-frames needs --clip (or --config)")
    if a.face_decimation and not (a.mesh_prep or a.config == 3):
        ap.error("--face-decimation needs --mesh-prep (or --config 3)")
    if a.decimate_borders != "fixed" and not a.face_decimation:
        ap.error("--decimate-borders needs --face-decimation")
    if a.field_grid and not a.face_decimation:
        ap.error("--field-grid needs --face-decimation (the extracted mesh has as many faces as the grid gives it)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    label = None
    if a.config == 1:
        a.clip, a.frames, a.steps = "davis_camel", 16, 50
        label = "configs[1]: davis_camel 16 frames, full 50-step scheduler, bf16, 1 x MI355X - PLUMBING on random-init weights, not the end-to-end metric"
    elif a.config == 3:
        a.clip, a.frames, a.steps, a.mesh_prep = "panda", 16, 50, True
        label = ("configs[3]: {video+3D}->4D panda path, 16 frames, 1 x MI355X - PLUMBING on random-init weights; differs from configs[1] only in the "
                 "anchor latent's source (Stage 0, reference path), which is seeded noise in both records, and in the mesh glue around Stage II "
                 "(dirty mesh -> merge_and_clean_mesh -> normalize_mesh -> sample_surface; denormalize_mesh + expand_to_original at the end)")
    if a.exact_fp32:
        print(json.dumps(run_exact_fp32(a.frames, a.steps, a.vertices, a.tiny, dev)))
        return
    print(json.dumps(run(a.frames, a.steps, a.vertices, a.tiny, dev, clip=a.clip, label=label, raw_frames=a.raw_frames,
                         features=a.features, mesh_prep=a.mesh_prep, face_decimation=a.face_decimation,
                         field_grid=a.field_grid, iso_method=a.iso_method, decimate_borders=a.decimate_borders)))


if __name__ == "__main__":
    main()
