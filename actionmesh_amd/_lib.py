"""ctypes binding of libactionmesh_amd.so (the C-ABI in include/actionmesh_amd.h).

The HIP library is the product.  There is NO CPU fallback: importing this module
never fails (so host-side logic stays testable without a GPU), but `lib()` raises
`HipLibraryMissing` when the shared object has not been built, and every compute
entry point raises `RuntimeError(am_last_error())` on a non-zero status.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# ACTIONMESH_AMD_LIB: another build of the same library (kernel A/B variants, tools/build_variants.sh); never a fallback
LIB_PATH = os.environ.get("ACTIONMESH_AMD_LIB") or os.path.join(_HERE, "libactionmesh_amd.so")
# The float16 build of the same sources (csrc/Makefile: -DAM_F16): same symbols, the 16-bit storage / MFMA element type is IEEE half.
# The reference CLI's `--dtype float16` (inference/video_to_animated_mesh.py:153,222).  Loaded on first use, never a fallback.
LIB_PATH_F16 = os.environ.get("ACTIONMESH_AMD_LIB_F16") or os.path.join(_HERE, "libactionmesh_amd_f16.so")
ABI_VERSION = 2      # 2 (round 5): am_peer_ring owns its events; am_peer_alloc_flags, am_peer_ring_destroy


class HipLibraryMissing(RuntimeError):
    pass


class AmConfig(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int32), ("num_layers", C.c_int32), ("num_heads", C.c_int32),
        ("width", C.c_int32), ("ff_inner", C.c_int32), ("cross_dim", C.c_int32),
        ("inflated_mask_lo", C.c_uint32), ("inflated_mask_hi", C.c_uint32),
        ("max_batch", C.c_int32), ("max_frames_local", C.c_int32), ("max_tokens", C.c_int32),
        ("max_ctx_tokens", C.c_int32), ("world_size", C.c_int32), ("rank", C.c_int32),
        ("attn_defer_log2", C.c_int32), ("attn_fp8", C.c_int32), ("reserved", C.c_int32 * 6),
    ]


# am_gemm_args.act: the activation code in the low byte; the bits above it are diagnostic and test switches, never product options
# (the AM_GEMM_* defines of include/actionmesh_amd.h; tests/test_host_cpu.py holds the two lists equal)
GEMM_ACT_MASK, GEMM_ACT_GELU = 0xff, 1
GEMM_FORCE_128, GEMM_LOCKSTEP, GEMM_FORCE_256 = 0x100, 0x200, 0x400
GEMM_ABLATE_STORE, GEMM_ABLATE_READ, GEMM_ABLATE_MASK = 0x800, 0x1000, 0x1800
GEMM_SKEW_SHIFT, GEMM_SKEW_MASK = 13, 0xe000
GEMM_NO_GELU_TABLE = 0x10000

# am_attn_args.defer_log2 and the row stride of am_attn_args.state (the AM_ATTN_* defines of include/actionmesh_amd.h, which explains
# them; tests/test_host_cpu.py holds the two lists equal)
ATTN_STATE_LD = 132
ATTN_REBASE_ALWAYS, ATTN_REBASE_DEFERRED = 0, 8
ATTN_4WAVE, ATTN_4X64, ATTN_BALANCED, ATTN_8WAVE, ATTN_4X64_DEFERRED = 50, 60, 70, 90, 28
ATTN_VARIANTS, ATTN_ABLATE_4X64 = 100, 3000
ATTN_FP8_ABLATE, ATTN_FP8_4X64, ATTN_FP8_8WAVE, ATTN_FP8_PRODUCT_ABLATE, ATTN_FP8_FAST = 5000, 5100, 5200, 5300, 5400


class AmGemmArgs(C.Structure):
    _fields_ = [
        ("A1", C.c_void_p), ("lda1", C.c_int32), ("K1", C.c_int32),
        ("A2", C.c_void_p), ("lda2", C.c_int32),
        ("W", C.c_void_p), ("ldw", C.c_int32),
        ("bias", C.c_void_p), ("residual", C.c_void_p),
        ("C", C.c_void_p), ("ldc", C.c_int32),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("act", C.c_int32),
        ("a_G", C.c_int32), ("a_gs", C.c_int32), ("a_off", C.c_int32),
        ("c_G", C.c_int32), ("c_gs", C.c_int32), ("c_off", C.c_int32),
        ("ln_stats", C.c_void_p), ("ln_colsum", C.c_void_p), ("ln_part", C.c_void_p),
    ]


class AmHeadPostArgs(C.Structure):
    _fields_ = [
        ("X", C.c_void_p), ("ldx", C.c_int32),
        ("rows", C.c_int64), ("seq_len", C.c_int32), ("rows_per_frame", C.c_int32),
        ("heads", C.c_int32), ("nparts", C.c_int32), ("kinds", C.c_int32 * 3),
        ("w_q", C.c_void_p), ("w_k", C.c_void_p), ("eps", C.c_float),
        ("rope_cos", C.c_void_p), ("rope_sin", C.c_void_p),
        ("out_q", C.c_void_p), ("sq_pad", C.c_int32),
        ("out_k", C.c_void_p), ("out_vt", C.c_void_p), ("sk_pad", C.c_int32),
    ]


class AmNnArgs(C.Structure):
    _fields_ = [
        ("points", C.c_void_p), ("n_points", C.c_int64), ("points_bstride", C.c_int64),
        ("queries", C.c_void_p), ("n_queries", C.c_int64), ("queries_bstride", C.c_int64),
        ("batch", C.c_int32), ("precise", C.c_int32),
        ("out_index", C.c_void_p), ("out_d2", C.c_void_p),
    ]


NN_GRID_MAX_CELLS = 128                    # AM_NN_GRID_MAX_CELLS
NN_GRID_BAD_ORDER, NN_GRID_BAD_CELL_START, NN_GRID_BAD_INDEX, NN_GRID_BAD_QUERY_ORDER = 1, 2, 4, 8     # the AM_NN_GRID_BAD_* flag bits


class AmNnGrid(C.Structure):               # am_nn_grid
    _fields_ = [
        ("n_points", C.c_int64), ("batch", C.c_int32), ("cells", C.c_int32),
        ("frame", C.c_void_p), ("slabs", C.c_void_p), ("cell_start", C.c_void_p), ("order", C.c_void_p), ("sorted", C.c_void_p),
    ]


class AmNnGridBuildArgs(C.Structure):      # am_nn_grid_build_args
    _fields_ = [
        ("points", C.c_void_p), ("points_bstride", C.c_int64), ("grid", AmNnGrid), ("out_cell", C.c_void_p), ("out_flag", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
    ]


class AmNnGridSearchArgs(C.Structure):     # am_nn_grid_search_args
    _fields_ = [
        ("grid", AmNnGrid), ("queries", C.c_void_p), ("n_queries", C.c_int64), ("queries_bstride", C.c_int64),
        ("batch", C.c_int32), ("precise", C.c_int32), ("query_order", C.c_void_p), ("query_order_bstride", C.c_int64),
        ("out_index", C.c_void_p), ("out_d2", C.c_void_p), ("out_flag", C.c_void_p),
    ]


ICP_NO_NEIGHBOUR = 1                       # AM_ICP_NO_NEIGHBOUR: am_icp_step's out_flag bit


class AmIcpArgs(C.Structure):              # am_icp_args
    _fields_ = [
        ("pred", C.c_void_p), ("gt", C.c_void_p), ("rot_init", C.c_void_p), ("n_pred", C.c_int64), ("n_gt", C.c_int64),
        ("batch", C.c_int32), ("update", C.c_int32),
        ("params", C.c_void_p), ("adam_m", C.c_void_p), ("adam_v", C.c_void_p), ("best", C.c_void_p),
        ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
        ("bias_correction1", C.c_double), ("bias_correction2", C.c_double),
        ("out_loss", C.c_void_p), ("out_rot", C.c_void_p), ("out_sums", C.c_void_p), ("out_grad", C.c_void_p), ("out_flag", C.c_void_p),
    ]


class AmAttnArgs(C.Structure):
    _fields_ = [
        ("Q", C.c_void_p), ("K", C.c_void_p), ("Vt", C.c_void_p), ("O", C.c_void_p),
        ("nseq", C.c_int32), ("heads", C.c_int32), ("sq", C.c_int32), ("sq_pad", C.c_int32),
        ("sk", C.c_int32), ("sk_pad", C.c_int32), ("nchunks", C.c_int32),
        ("chunk_stride", C.c_int64), ("ldo", C.c_int32), ("scale", C.c_float),
        ("defer_log2", C.c_int32),
        ("chunk_first", C.c_int32), ("chunk_total", C.c_int32), ("rows", C.c_int32), ("state_mode", C.c_int32),
        ("state", C.c_void_p),
    ]


class AmAttnF32Args(C.Structure):      # am_attn_f32_args
    _fields_ = [
        ("Q", C.c_void_p), ("ldq", C.c_int64), ("q_off", C.c_int32), ("q_hs", C.c_int32),
        ("K", C.c_void_p), ("ldk", C.c_int64), ("k_off", C.c_int32), ("k_hs", C.c_int32),
        ("V", C.c_void_p), ("ldv", C.c_int64), ("v_off", C.c_int32), ("v_hs", C.c_int32),
        ("O", C.c_void_p), ("ldo", C.c_int64),
        ("nseq", C.c_int32), ("heads", C.c_int32), ("sq", C.c_int32), ("sk", C.c_int32), ("head_dim", C.c_int32),
        ("scale", C.c_float),
    ]


RENDER_MAX_CAMERAS = 16


class AmRenderCamera(C.Structure):     # am_render_camera
    _fields_ = [("R", C.c_float * 9), ("T", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("px", C.c_float), ("py", C.c_float)]


class AmRenderArgs(C.Structure):       # am_render_args
    _fields_ = [
        ("verts", C.c_void_p), ("faces", C.c_void_p), ("offsets", C.c_void_p), ("corners", C.c_void_p),
        ("n_frames", C.c_int32), ("n_verts", C.c_int32), ("n_faces", C.c_int32), ("n_cameras", C.c_int32),
        ("cameras", AmRenderCamera * RENDER_MAX_CAMERAS), ("image_size", C.c_int32),
        ("out_rgba", C.c_void_p), ("out_mask", C.c_void_p), ("out_normal", C.c_void_p),
        ("out_face", C.c_void_p), ("out_bary", C.c_void_p), ("out_flag", C.c_void_p),
    ]


FPS_F32, FPS_F16, FPS_BF16 = 0, 1, 2    # am_fps_args.dtype


class AmFpsArgs(C.Structure):          # am_fps_args
    _fields_ = [
        ("points", C.c_void_p), ("dtype", C.c_int32), ("batch", C.c_int32), ("n_points", C.c_int64),
        ("dims", C.c_int32), ("dist_dims", C.c_int32), ("batch_stride", C.c_int64), ("point_stride", C.c_int64),
        ("n_samples", C.c_int64), ("start_idx", C.c_void_p), ("out_index", C.c_void_p), ("out_dist", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("threads", C.c_int32), ("reserved", C.c_int32),
    ]


class AmImageFrame(C.Structure):       # am_image_frame
    _fields_ = [
        ("src_offset", C.c_int64), ("dst_offset", C.c_int64), ("src_w", C.c_int32), ("src_h", C.c_int32),
        ("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("pad_x", C.c_int32), ("pad_y", C.c_int32),
        ("htab", C.c_int32), ("vtab", C.c_int32), ("left", C.c_int32), ("top", C.c_int32), ("row_lo", C.c_int32), ("n_rows", C.c_int32),
    ]


class AmImageAlphaStatsArgs(C.Structure):      # am_image_alpha_stats_args
    _fields_ = [("rgba", C.c_void_p), ("n_frames", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("reserved", C.c_int32),
                ("out_stats", C.c_void_p)]


class AmImageResampleArgs(C.Structure):        # am_image_resample_args
    _fields_ = [
        ("src", C.c_void_p), ("src_bytes", C.c_int64), ("src_channels", C.c_int32), ("fill", C.c_int32), ("composite", C.c_void_p),
        ("n_frames", C.c_int32), ("out_w", C.c_int32), ("out_h", C.c_int32), ("reserved", C.c_int32),
        ("frames", C.c_void_p), ("frames_dev", C.c_void_p), ("taps", C.c_void_p), ("taps_dev", C.c_void_p), ("taps_len", C.c_int64),
        ("norm_table", C.c_void_p), ("out_pixels", C.c_void_p), ("out_u8", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
    ]


class AmImageMaterializeArgs(C.Structure):     # am_image_materialize_args
    _fields_ = [
        ("src", C.c_void_p), ("src_bytes", C.c_int64), ("src_channels", C.c_int32), ("fill", C.c_int32), ("composite", C.c_void_p),
        ("n_frames", C.c_int32), ("reserved", C.c_int32), ("frames", C.c_void_p), ("frames_dev", C.c_void_p),
        ("out", C.c_void_p), ("out_bytes", C.c_int64),
    ]


class AmMaskRefineArgs(C.Structure):           # am_mask_refine_args
    _fields_ = [
        ("mask", C.c_void_p), ("n_frames", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("min_size", C.c_int32),
        ("threshold", C.c_int32), ("reserved", C.c_int32), ("out_mask", C.c_void_p), ("out_labels", C.c_void_p), ("out_stats", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
    ]


class AmGraphArgs(C.Structure):                # am_graph_args
    _fields_ = [
        ("n_nodes", C.c_int64), ("n_edges", C.c_int64), ("edges", C.c_void_p), ("out_label", C.c_void_p), ("out_size", C.c_void_p),
        ("out_flag", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
    ]


class AmVertexNormalsArgs(C.Structure):        # am_vertex_normals_args
    _fields_ = [
        ("vertices", C.c_void_p), ("vertices_f64", C.c_int32), ("n_frames", C.c_int32), ("n_vertices", C.c_int64), ("n_faces", C.c_int64),
        ("frame_stride", C.c_int64), ("faces", C.c_void_p), ("offsets", C.c_void_p), ("corners", C.c_void_p),
        ("out_features", C.c_void_p), ("out_normals", C.c_void_p), ("out_face_normals", C.c_void_p), ("out_flag", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
    ]


class AmFaceAreasArgs(C.Structure):            # am_face_areas_args
    _fields_ = [
        ("vertices", C.c_void_p), ("vertices_f64", C.c_int32), ("reserved", C.c_int32), ("n_vertices", C.c_int64), ("n_faces", C.c_int64),
        ("faces", C.c_void_p), ("out_areas", C.c_void_p), ("out_flag", C.c_void_p),
    ]


class AmSurfaceSampleArgs(C.Structure):        # am_surface_sample_args
    _fields_ = [
        ("vertices", C.c_void_p), ("vertices_f64", C.c_int32), ("reserved", C.c_int32), ("n_vertices", C.c_int64), ("n_faces", C.c_int64),
        ("n_samples", C.c_int64), ("faces", C.c_void_p), ("cdf", C.c_void_p), ("u_face", C.c_void_p), ("u_bary", C.c_void_p),
        ("out_points", C.c_void_p), ("out_face_index", C.c_void_p), ("out_normals", C.c_void_p), ("out_flag", C.c_void_p),
    ]


DECIMATE_NO_KEY = 2 ** 63 - 1               # AM_DECIMATE_NO_KEY
MESH_BAD_FACE, MESH_BAD_CSR = 1, 2          # the out_flag bits of am_vertex_normals / am_face_areas / am_surface_sample / am_render_normals
DECIMATE_BAD_FACE, DECIMATE_BAD_CSR, DECIMATE_BAD_EDGE, DECIMATE_BAD_KEPT = MESH_BAD_FACE, MESH_BAD_CSR, 4, 8      # am_decimate_*'s out_flag bits


class AmDecimateQuadricsArgs(C.Structure):     # am_decimate_quadrics_args
    _fields_ = [
        ("positions", C.c_void_p), ("n_vertices", C.c_int64), ("n_faces", C.c_int64), ("faces", C.c_void_p), ("offsets", C.c_void_p),
        ("corners", C.c_void_p), ("out_quadrics", C.c_void_p), ("out_flag", C.c_void_p),
    ]


class AmDecimateEdgesArgs(C.Structure):        # am_decimate_edges_args
    _fields_ = [
        ("positions", C.c_void_p), ("quadrics", C.c_void_p), ("n_vertices", C.c_int64), ("n_faces", C.c_int64), ("n_edges", C.c_int64),
        ("faces", C.c_void_p), ("offsets", C.c_void_p), ("corners", C.c_void_p), ("edges", C.c_void_p), ("half_edge_to_edge", C.c_void_p),
        ("edge_count", C.c_void_p), ("out_positions", C.c_void_p), ("out_cost", C.c_void_p), ("out_key", C.c_void_p),
        ("out_flag", C.c_void_p),
    ]


class AmDecimateSelectArgs(C.Structure):       # am_decimate_select_args
    _fields_ = [
        ("n_vertices", C.c_int64), ("n_faces", C.c_int64), ("n_edges", C.c_int64), ("faces", C.c_void_p), ("offsets", C.c_void_p),
        ("corners", C.c_void_p), ("edges", C.c_void_p), ("half_edge_to_edge", C.c_void_p), ("keys", C.c_void_p), ("out_m1", C.c_void_p),
        ("out_m2", C.c_void_p), ("out_selected", C.c_void_p), ("out_flag", C.c_void_p),
    ]


class AmDecimateApplyArgs(C.Structure):        # am_decimate_apply_args
    _fields_ = [
        ("n_vertices", C.c_int64), ("n_faces", C.c_int64), ("n_edges", C.c_int64), ("n_kept", C.c_int64), ("kept", C.c_void_p),
        ("edges", C.c_void_p), ("candidates", C.c_void_p), ("offsets", C.c_void_p), ("corners", C.c_void_p), ("positions", C.c_void_p),
        ("quadrics", C.c_void_p), ("faces", C.c_void_p), ("vertex_map", C.c_void_p), ("out_face_dead", C.c_void_p),
        ("out_flag", C.c_void_p),
    ]


class AmDecimateBorderQuadricsArgs(C.Structure):       # am_decimate_border_quadrics_args
    _fields_ = [
        ("positions", C.c_void_p), ("n_vertices", C.c_int64), ("n_faces", C.c_int64), ("n_edges", C.c_int64), ("faces", C.c_void_p),
        ("offsets", C.c_void_p), ("corners", C.c_void_p), ("half_edge_to_edge", C.c_void_p), ("edge_count", C.c_void_p),
        ("border_weight", C.c_double), ("out_quadrics", C.c_void_p), ("out_flag", C.c_void_p),
    ]


class AmDecimateBorderEdgesArgs(C.Structure):  # am_decimate_border_edges_args: the fields of am_decimate_edges_args
    _fields_ = list(AmDecimateEdgesArgs._fields_)


ISO_BAD_VERTEX_OFFSET, ISO_BAD_TRI_OFFSET, ISO_BAD_TABLE = 1, 2, 4      # am_iso_vertices' / am_iso_triangles' out_flag bits


class AmIsoClassifyArgs(C.Structure):          # am_iso_classify_args
    _fields_ = [
        ("values", C.c_void_p), ("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64), ("level", C.c_double),
        ("inside_above", C.c_int32), ("reserved", C.c_int32), ("out_mask", C.c_void_p), ("out_count", C.c_void_p),
    ]


class AmIsoVerticesArgs(C.Structure):          # am_iso_vertices_args
    _fields_ = [
        ("values", C.c_void_p), ("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64), ("level", C.c_double),
        ("origin", C.c_double * 3), ("spacing", C.c_double * 3), ("mask", C.c_void_p), ("vertex_offset", C.c_void_p),
        ("n_vertices", C.c_int64), ("out_vertices", C.c_void_p), ("out_flag", C.c_void_p),
    ]


class AmIsoTrianglesArgs(C.Structure):         # am_iso_triangles_args
    _fields_ = [
        ("values", C.c_void_p), ("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64), ("level", C.c_double),
        ("inside_above", C.c_int32), ("reserved", C.c_int32), ("mask", C.c_void_p), ("count", C.c_void_p),
        ("vertex_offset", C.c_void_p), ("tri_offset", C.c_void_p), ("n_vertices", C.c_int64), ("n_triangles", C.c_int64),
        ("out_faces", C.c_void_p), ("out_flag", C.c_void_p),
    ]


DMC_BAD_VERTEX_OFFSET, DMC_BAD_TRI_OFFSET, DMC_BAD_CODE = 1, 2, 4      # am_dmc_vertices' / am_dmc_triangles' out_flag bits


class AmDmcCellsArgs(C.Structure):             # am_dmc_cells_args
    _fields_ = [
        ("values", C.c_void_p), ("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64), ("level", C.c_double),
        ("inside_above", C.c_int32), ("reserved", C.c_int32), ("out_config", C.c_void_p), ("out_double", C.c_void_p),
    ]


class AmDmcClassifyArgs(C.Structure):          # am_dmc_classify_args
    _fields_ = [
        ("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64), ("config", C.c_void_p), ("double_faces", C.c_void_p),
        ("out_code", C.c_void_p), ("out_count", C.c_void_p), ("out_edge_mask", C.c_void_p),
    ]


class AmDmcVerticesArgs(C.Structure):          # am_dmc_vertices_args
    _fields_ = [
        ("values", C.c_void_p), ("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64), ("level", C.c_double),
        ("origin", C.c_double * 3), ("spacing", C.c_double * 3), ("inside_above", C.c_int32), ("reserved", C.c_int32),
        ("code", C.c_void_p), ("vertex_offset", C.c_void_p), ("n_vertices", C.c_int64), ("out_vertices", C.c_void_p),
        ("out_flag", C.c_void_p),
    ]


class AmDmcTrianglesArgs(C.Structure):         # am_dmc_triangles_args
    _fields_ = [
        ("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64), ("code", C.c_void_p), ("edge_mask", C.c_void_p),
        ("vertex_offset", C.c_void_p), ("tri_offset", C.c_void_p), ("vertices", C.c_void_p), ("n_vertices", C.c_int64),
        ("n_triangles", C.c_int64), ("out_faces", C.c_void_p), ("out_flag", C.c_void_p),
    ]


PEER_MAX_RANKS = 16


class AmPeerRing(C.Structure):          # include/actionmesh_amd_sharded.h
    _fields_ = [
        ("world", C.c_int32), ("rank", C.c_int32), ("chunk_bytes", C.c_uint64),
        ("kv", C.c_void_p), ("flags", C.c_void_p),
        ("peer_kv", C.c_void_p * PEER_MAX_RANKS), ("peer_flags", C.c_void_p * PEER_MAX_RANKS),
        ("side_stream", C.c_void_p), ("seq", C.c_uint32),
        ("ev_fork", C.c_void_p), ("ev_pushed", C.c_void_p),
    ]


# every struct include/*.h declares: C typedef name -> ctypes mirror (tests/test_host_cpu.py compares the names with the headers and
# every size and field offset with what a C compiler makes of them)
STRUCTS = {
    "am_config": AmConfig, "am_gemm_args": AmGemmArgs, "am_headpost_args": AmHeadPostArgs, "am_attn_args": AmAttnArgs,
    "am_attn_f32_args": AmAttnF32Args, "am_nn_args": AmNnArgs, "am_nn_grid": AmNnGrid, "am_nn_grid_build_args": AmNnGridBuildArgs,
    "am_nn_grid_search_args": AmNnGridSearchArgs, "am_icp_args": AmIcpArgs, "am_render_camera": AmRenderCamera, "am_render_args": AmRenderArgs,
    "am_fps_args": AmFpsArgs, "am_image_frame": AmImageFrame, "am_image_alpha_stats_args": AmImageAlphaStatsArgs,
    "am_image_resample_args": AmImageResampleArgs, "am_image_materialize_args": AmImageMaterializeArgs,
    "am_mask_refine_args": AmMaskRefineArgs, "am_graph_args": AmGraphArgs, "am_vertex_normals_args": AmVertexNormalsArgs,
    "am_face_areas_args": AmFaceAreasArgs, "am_surface_sample_args": AmSurfaceSampleArgs,
    "am_decimate_quadrics_args": AmDecimateQuadricsArgs, "am_decimate_edges_args": AmDecimateEdgesArgs,
    "am_decimate_select_args": AmDecimateSelectArgs, "am_decimate_apply_args": AmDecimateApplyArgs,
    "am_decimate_border_quadrics_args": AmDecimateBorderQuadricsArgs, "am_decimate_border_edges_args": AmDecimateBorderEdgesArgs,
    "am_iso_classify_args": AmIsoClassifyArgs, "am_iso_vertices_args": AmIsoVerticesArgs, "am_iso_triangles_args": AmIsoTrianglesArgs,
    "am_dmc_cells_args": AmDmcCellsArgs, "am_dmc_classify_args": AmDmcClassifyArgs, "am_dmc_vertices_args": AmDmcVerticesArgs,
    "am_dmc_triangles_args": AmDmcTrianglesArgs,
    "am_peer_ring": AmPeerRing,
}

# every symbol include/*.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "am_last_error": (C.c_char_p, []),
    "am_abi_version": (C.c_int, []),
    "am_create": (C.c_int, [C.POINTER(AmConfig), C.POINTER(_P)]),
    "am_destroy": (C.c_int, [_P]),
    "am_load_weight": (C.c_int, [_P, C.c_char_p, _P, C.c_size_t]),
    "am_weights_missing": (C.c_int, [_P]),
    "am_set_context": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "am_set_branch_hints": (C.c_int, [_P, _P, C.c_int]),
    "am_denoise_forward": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "am_denoise_forward_graph": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "am_graph_stats": (C.c_int, [_P, _P]),
    "am_forward_begin": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "am_point_embed": (C.c_int, [_P, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P]),
    "am_displacement": (C.c_int, [_P, C.c_int, C.c_int64, C.c_int, _P, _P]),
    "am_attention_fallback_count": (C.c_int, [_P]),
    "am_patchify": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P]),
    "am_gemm_f32": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64, _P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "am_attention_f32": (C.c_int, [C.POINTER(AmAttnF32Args), _P]),
    "am_layernorm_f32": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int, C.c_float, _P]),
    "am_point_embed_f32": (C.c_int, [_P, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P]),
    "am_patchify_f32": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P]),
    "am_displacement_f32": (C.c_int, [_P, C.c_int, C.c_int64, C.c_int, _P, _P]),
    "am_head_post_f32": (C.c_int, [_P, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int, _P, C.c_float, _P, _P, C.c_int, C.c_int, _P]),
    "am_rope_f32": (C.c_int, [_P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, _P, _P, C.c_int, C.c_int, _P]),
    "am_flow_step_f32": (C.c_int, [_P, _P, C.c_int, _P, C.c_float, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P]),
    "am_nn_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "am_nn_search": (C.c_int, [C.POINTER(AmNnArgs), _P, C.c_size_t, _P]),
    "am_nn_grid_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "am_nn_grid_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "am_nn_grid_cells": (C.c_int, [C.POINTER(AmNnGridBuildArgs), _P]),
    "am_nn_grid_build": (C.c_int, [C.POINTER(AmNnGridBuildArgs), _P]),
    "am_nn_grid_search": (C.c_int, [C.POINTER(AmNnGridSearchArgs), _P]),
    "am_icp_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int]),
    "am_icp_step": (C.c_int, [C.POINTER(AmIcpArgs), _P, C.c_size_t, _P]),
    "am_render_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "am_render_normals": (C.c_int, [C.POINTER(AmRenderArgs), _P, C.c_size_t, _P]),
    "am_fps_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "am_fps": (C.c_int, [C.POINTER(AmFpsArgs), _P]),
    "am_image_alpha_stats": (C.c_int, [C.POINTER(AmImageAlphaStatsArgs), _P]),
    "am_image_resample_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "am_image_resample": (C.c_int, [C.POINTER(AmImageResampleArgs), _P]),
    "am_image_materialize": (C.c_int, [C.POINTER(AmImageMaterializeArgs), _P]),
    "am_mask_refine_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "am_mask_refine": (C.c_int, [C.POINTER(AmMaskRefineArgs), _P]),
    "am_graph_components_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "am_graph_components": (C.c_int, [C.POINTER(AmGraphArgs), _P]),
    "am_vertex_normals_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int64]),
    "am_vertex_normals": (C.c_int, [C.POINTER(AmVertexNormalsArgs), _P]),
    "am_face_areas": (C.c_int, [C.POINTER(AmFaceAreasArgs), _P]),
    "am_surface_sample": (C.c_int, [C.POINTER(AmSurfaceSampleArgs), _P]),
    "am_decimate_quadrics": (C.c_int, [C.POINTER(AmDecimateQuadricsArgs), _P]),
    "am_decimate_edges": (C.c_int, [C.POINTER(AmDecimateEdgesArgs), _P]),
    "am_decimate_select": (C.c_int, [C.POINTER(AmDecimateSelectArgs), _P]),
    "am_decimate_apply": (C.c_int, [C.POINTER(AmDecimateApplyArgs), _P]),
    "am_decimate_border_quadrics": (C.c_int, [C.POINTER(AmDecimateBorderQuadricsArgs), _P]),
    "am_decimate_border_edges": (C.c_int, [C.POINTER(AmDecimateBorderEdgesArgs), _P]),
    "am_iso_classify": (C.c_int, [C.POINTER(AmIsoClassifyArgs), _P]),
    "am_iso_vertices": (C.c_int, [C.POINTER(AmIsoVerticesArgs), _P]),
    "am_iso_triangles": (C.c_int, [C.POINTER(AmIsoTrianglesArgs), _P]),
    "am_dmc_cells": (C.c_int, [C.POINTER(AmDmcCellsArgs), _P]),
    "am_dmc_classify": (C.c_int, [C.POINTER(AmDmcClassifyArgs), _P]),
    "am_dmc_vertices": (C.c_int, [C.POINTER(AmDmcVerticesArgs), _P]),
    "am_dmc_triangles": (C.c_int, [C.POINTER(AmDmcTrianglesArgs), _P]),
    "am_layer_pre_attn": (C.c_int, [_P, C.c_int, _P]),
    "am_layer_attn_local": (C.c_int, [_P, C.c_int, _P]),
    "am_layer_post_attn": (C.c_int, [_P, C.c_int, _P]),
    "am_forward_end": (C.c_int, [_P, _P, _P]),
    "am_kv_chunk_elems": (C.c_int, [_P, C.POINTER(C.c_size_t)]),
    "am_bind_kv_buffers": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "am_bind_kv8_buffers": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "am_attention_counters": (C.c_int, [_P, _P]),
    "am_flow_step": (C.c_int, [_P, _P, C.c_int, _P, C.c_float, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P]),
    "am_step_flops": (C.c_double, [_P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "am_gemm_bf16": (C.c_int, [C.POINTER(AmGemmArgs), _P]),
    "am_layernorm_bf16": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int, C.c_float, _P]),
    "am_add_layernorm_f32": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_int, C.c_float, _P]),
    "am_row_stats_bf16": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_float, _P]),
    "am_row_stats_finalize": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int64, C.c_float, _P]),
    "am_layernorm_stats_bf16": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int, C.c_float, _P, _P]),
    "am_ln_fold_weight": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "am_head_post": (C.c_int, [C.POINTER(AmHeadPostArgs), _P]),
    "am_gemm_headpost_bf16": (C.c_int, [C.POINTER(AmGemmArgs), C.POINTER(AmHeadPostArgs), _P]),
    "am_attention_bf16": (C.c_int, [C.POINTER(AmAttnArgs), _P]),
    "am_attention_quantize_fp8": (C.c_int, [C.POINTER(AmAttnArgs), _P, _P, _P, _P]),
    "am_attention_fp8": (C.c_int, [C.POINTER(AmAttnArgs), _P, _P, _P, _P]),
    "am_peer_alloc": (C.c_int, [C.c_size_t, C.POINTER(_P)]),
    "am_peer_alloc_flags": (C.c_int, [C.c_size_t, C.POINTER(_P), C.POINTER(C.c_int)]),
    "am_peer_free": (C.c_int, [_P]),
    "am_peer_export": (C.c_int, [_P, _P]),
    "am_peer_open": (C.c_int, [_P, C.POINTER(_P)]),
    "am_peer_close": (C.c_int, [_P]),
    "am_peer_copy": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "am_peer_signal": (C.c_int, [_P, C.c_uint32, _P]),
    "am_peer_wait": (C.c_int, [_P, C.c_uint32, _P, _P]),
    "am_debug_trace_begin": (C.c_int, [_P, C.c_int]),
    "am_debug_trace_end": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int)]),
    "am_debug_trace_stage_name": (C.c_char_p, [C.c_int]),
    "am_f32_to_bf16": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "am_bf16_to_f32": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "am_timestep_sinusoid": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "am_forward_sharded_peer": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.POINTER(AmPeerRing), _P, C.c_int, _P]),
    "am_peer_ring_destroy": (C.c_int, [C.POINTER(AmPeerRing)]),
}

_libs = {}


def lib(kind: str = "bf16") -> C.CDLL:
    """Load (once) and return the shared library of the given 16-bit type ("bf16": the product default; "f16": the float16 build);
    fail loudly if it is absent."""
    if kind in _libs:
        return _libs[kind]
    if kind not in ("bf16", "f16"):
        raise ValueError(f"actionmesh_amd._lib.lib: kind must be 'bf16' or 'f16', got {kind!r}")
    path = LIB_PATH if kind == "bf16" else LIB_PATH_F16
    if not os.path.exists(path):
        raise HipLibraryMissing(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C actionmesh_amd/csrc`.  actionmesh_amd has no CPU fallback."
        )
    l = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(l, name)   # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if l.am_abi_version() != ABI_VERSION:
        raise HipLibraryMissing(f"ABI mismatch: library {l.am_abi_version()} != binding {ABI_VERSION}; rebuild")
    _libs[kind] = l
    return l


def kind_of(dtype) -> str:
    """'bf16' / 'f16' for torch.bfloat16 / torch.float16 (or their names); anything else is an error.  These are the two builds of the
    library; float32 is not a third build: the exact-fp32 entry points (am_gemm_f32, am_attention_f32, ...) live in both, and the modules
    that offer an fp32 mode (HipAutoencoder(cross_fp32=True) / (exact_fp32=True), HipImageEncoder(dtype="float32"),
    HipDenoiser(dtype="float32")) handle it before calling this (is_f32)."""
    name = str(dtype).replace("torch.", "")
    if name in ("bfloat16", "bf16"):
        return "bf16"
    if name in ("float16", "half", "f16", "fp16"):
        return "f16"
    raise ValueError(f"actionmesh_amd: the 16-bit type must be bfloat16 or float16, got {dtype!r}")


def is_f32(dtype) -> bool:
    """True for torch.float32 and its spellings: the dtype that selects a module's exact-fp32 mode."""
    return str(dtype).replace("torch.", "") in ("float32", "float", "fp32", "f32")


def autocast_kind(pinned: Optional[str] = None) -> str:
    """'bf16' or 'f16' for a module called like the reference's: the pinned kind if there is one, else the dtype of the caller's
    torch.autocast("cuda", dtype) region - the reference pipeline runs Stage I and Stage II inside one (pipeline.py:671, 679) with the
    CLI's --dtype {bfloat16, float16} - and bfloat16 outside any region.  float16 is chosen only when the caller asked for it."""
    if pinned is not None:
        return pinned
    import torch
    if hasattr(torch, "get_autocast_dtype"):
        enabled, dt = torch.is_autocast_enabled("cuda"), torch.get_autocast_dtype("cuda")
    else:                                    # older torch: the per-device getters (no silent bf16 under autocast(float16))
        enabled, dt = torch.is_autocast_enabled(), torch.get_autocast_gpu_dtype()
    return "f16" if (enabled and dt == torch.float16) else "bf16"


def torch_dtype(kind: str):
    import torch
    return torch.float16 if kind == "f16" else torch.bfloat16


def check(status: int, what: str = "", l: Optional[C.CDLL] = None) -> None:
    if status != 0:
        msg = (l if l is not None else lib()).am_last_error().decode(errors="replace")
        raise RuntimeError(f"libactionmesh_amd {what} failed (status {status}): {msg}")
