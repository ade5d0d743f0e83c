"""ctypes binding of ``libgd_raster.so`` (C-ABI declared in ``include/gd_raster.h``).

There is deliberately NO fallback: if the HIP library is missing or fails to load, every
entry point raises.  (The CPU oracle under ``oracle/`` is test infrastructure and is never
imported from this package.)
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libgd_raster.so")
_lib = None


def use_library(path: str) -> None:
    """Point the binding at another build of libgd_raster.so BEFORE its first use -- same-box A/B timing of experimental
    builds by the scripts under tools/ (tools/ablib.py) and ``bench.py --raster-lib``; the package itself reads no
    environment variable for this."""
    global _LIB_PATH
    if _lib is not None:
        raise RuntimeError("libgd_raster.so is already loaded")
    _LIB_PATH = os.path.abspath(path)


GD_MAX_VIEWS = 16
ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)

_vp = C.c_void_p
_i = C.c_int
_f = C.c_float


class Layout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in (
        "depths", "clamped", "radii", "means2D", "cov3D", "conic_opacity", "rgb", "tiles_touched", "point_offsets",
        "block_sums", "ranges", "n_contrib", "pair_counts", "point_list", "point_list_alt", "keys", "keys_alt", "sort_hist")]


# symbol -> (restype, argtypes); mirrors include/gd_raster.h one to one
_PF = C.POINTER(_f)
SIGNATURES = {
    "gd_raster_geom_bytes": (C.c_size_t, [_i, _i]),
    "gd_raster_image_bytes": (C.c_size_t, [_i, _i, _i]),
    "gd_raster_binning_bytes": (C.c_size_t, [C.c_int64]),
    "gd_raster_backward_scratch_bytes": (C.c_size_t, [_i, _i, C.c_int64]),
    "gd_raster_forward": (_i, [_vp] + [ALLOC_FN, _vp] * 3      # stream, 3 x (allocator, user)
                          + [_i] * 3 + [_vp] + [_i] * 2          # P D M, background, width height
                          + [_vp] * 5 + [_f] + [_vp] * 5         # means3D shs colors opac scales | mod | rot cov view proj campos
                          + [_f] * 2 + [_i] + [_vp] * 4 + [_i]), # tanx tany, prefiltered, color depth alpha radii, debug
    "gd_raster_backward": (_i, [_vp] + [_i] * 4 + [_vp] + [_i] * 2  # stream, P D M R, background, width height
                           + [_vp] * 5 + [_f] + [_vp] * 5            # means3D shs colors alphas scales | mod | rot cov view proj campos
                           + [_f] * 2 + [_vp] * 5                     # tanx tany, radii geom binning image bwd_scratch
                           + [_vp] * 3 + [_vp] * 10 + [_i]),          # dL_dpix/depth/alpha, 10 outputs, debug
    "gd_raster_mark_visible": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "gd_raster_forward_batched": (_i, [_vp, _i] + [ALLOC_FN, _vp] * 3
                                  + [_i] * 3 + [_vp] + [_i] * 2
                                  + [_vp] * 5 + [_f] + [_vp] * 5
                                  + [_PF] * 2 + [_i] + [_vp] * 4 + [_i]),
    "gd_raster_forward_batched_capacity": (_i, [_vp, _i] + [ALLOC_FN, _vp] * 3
                                           + [_i] * 3 + [_vp] + [_i] * 2
                                           + [_vp] * 5 + [_f] + [_vp] * 5
                                           + [_PF] * 2 + [_i] + [_vp] * 4 + [_i] + [C.c_int64, _vp]),   # + capacity, count_dev
    "gd_raster_backward_batched": (_i, [_vp, _i] + [_i] * 4 + [_vp] + [_i] * 2
                                   + [_vp] * 5 + [_f] + [_vp] * 5
                                   + [_PF] * 2 + [_vp] * 5
                                   + [_vp] * 3 + [_vp] * 8 + [_i]),   # 8 outputs (no dL_dconic / dL_ddepth)
    "gd_raster_get_layout": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, C.c_int64, C.POINTER(Layout)]),
    "gd_raster_sort_bits": (_i, [_i, _i, _i]),
    "gd_raster_blend_exp": (_i, [C.c_void_p, C.c_void_p, C.c_void_p, _i]),
    "gd_raster_profile_enable": (_i, [_i]),
    "gd_raster_profile_collect": (_i, []),
    "gd_raster_force_binning": (_i, [_i]),
    "gd_raster_poison_lds": (_i, [_vp]),
    "gd_raster_profile_get": (_i, [_i, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "gd_raster_profile_reset": (_i, []),
    "gd_raster_profile_kernel_name": (C.c_char_p, [_i]),
    "gd_raster_last_error": (C.c_char_p, []),
    "gd_raster_build_info": (C.c_char_p, []),
}
# scene-side kernels in the same library (include/gd_scene.h)
_I64P = C.POINTER(C.c_int64)
SCENE_SIGNATURES = {
    "gd_scene_dist2_scratch_bytes": (C.c_size_t, [_i]),
    "gd_scene_dist2": (_i, [_vp, _i, _vp, _vp, _vp]),
    "gd_scene_adam_step": (_i, [_vp, _vp, _vp, _vp, _vp, C.c_int64, _i, _I64P, C.POINTER(C.c_double), C.c_double,
                                C.c_double, C.c_double, _i]),
    "gd_scene_densify_stats": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "gd_scene_activate_forward": (_i, [_vp, _i, _i] + [_vp] * 9),
    "gd_scene_activate_backward": (_i, [_vp, _i, _i] + [_vp] * 12),
    "gd_scene_densify_scratch_bytes": (C.c_size_t, [_i]),
    "gd_scene_densify_plan": (_i, [_vp, _i, _vp, _vp, _vp, _vp, C.c_float, C.c_float, C.c_float, C.c_float, _vp,
                                   C.POINTER(C.c_uint32)]),
    "gd_scene_densify_apply": (_i, [_vp, _i, _i, C.POINTER(C.c_int), _i, _i, _i, C.POINTER(C.c_uint32)] + [_vp] * 8),
    "gd_scene_densify_last_error": (C.c_char_p, []),
    "gd_scene_shell_grid": (_i, [_PF, _PF, _f, _PF, C.POINTER(_i)]),
    "gd_scene_shell_scratch_bytes": (C.c_size_t, [_i, C.c_int64]),
    "gd_scene_shell_search": (_i, [_vp, _i, _vp, _i, _vp, _PF, _PF, _f, _vp, _vp, _vp]),
    "gd_scene_last_error": (C.c_char_p, []),
}
# mesh render path of the NeTF stage in the same library (include/gd_mesh.h)
MESH_SIGNATURES = {
    "gd_mesh_rasterize_scratch_bytes": (C.c_size_t, [_i] * 3),
    "gd_mesh_rasterize": (_i, [_vp] + [_i] * 4 + [_vp] * 4),                       # stream, V F H W, pos tri rast scratch
    "gd_mesh_interpolate_forward": (_i, [_vp] + [_i] * 5 + [_vp] * 4),             # stream, V F C H W, attr rast tri out
    "gd_mesh_interpolate_backward_scratch_bytes": (C.c_size_t, [_i] * 2),
    "gd_mesh_interpolate_backward": (_i, [_vp] + [_i] * 5 + [_vp] * 8),            # ..., pos tri rast dout ptr idx dattr scratch
    "gd_mesh_antialias_weights": (_i, [_vp] + [_i] * 4 + [_vp] * 5),               # stream, V F H W, rast pos tri opp wts
    "gd_mesh_antialias_apply": (_i, [_vp] + [_i] * 3 + [_vp] * 3 + [_i]),          # stream, C H W, in wts out, adjoint
    "gd_mesh_last_error": (C.c_char_p, []),
}


# its moving-geometry side: gradients to vertex positions and the visible-vertex mask (include/gd_mesh_deform.h)
MESH_DEFORM_SIGNATURES = {
    "gd_mesh_interpolate_backward_rast": (_i, [_vp] + [_i] * 5 + [_vp] * 5),       # stream, V F C H W, attr rast tri dout drast
    "gd_mesh_rasterize_backward_scratch_bytes": (C.c_size_t, [_i]),
    "gd_mesh_rasterize_backward": (_i, [_vp] + [_i] * 4 + [_vp] * 8),              # ..., pos tri rast drast ptr idx dpos scratch
    "gd_mesh_antialias_backward_pos_scratch_bytes": (C.c_size_t, [_i]),
    "gd_mesh_antialias_backward_pos": (_i, [_vp] + [_i] * 5 + [_vp] * 10),         # stream, V F C H W, rast pos tri opp in dout ptr idx dpos scratch
    "gd_mesh_visible_vertices": (_i, [_vp] + [_i] * 3 + [_vp] * 3),                # stream, V F npix, rast tri vis
}

# the deformer's geometry terms: normals, uniform Laplacian and normal consistency (include/gd_mesh_geometry.h)
MESH_GEOMETRY_SIGNATURES = {
    "gd_mesh_normals_forward": (_i, [_vp] + [_i] * 2 + [_vp] * 7),                 # stream, V F, verts tri ptr idx fn vn len
    "gd_mesh_normals_backward_scratch_bytes": (C.c_size_t, [_i]),
    "gd_mesh_normals_backward": (_i, [_vp] + [_i] * 2 + [_vp] * 10),               # ..., verts tri ptr idx vn len dvn dfn dverts scratch
    "gd_mesh_loss_scratch_bytes": (C.c_size_t, [_i]),
    "gd_mesh_laplacian_forward": (_i, [_vp] + [_i] * 2 + [_vp] * 6),               # stream, V N, verts ptr idx delta loss scratch
    "gd_mesh_laplacian_backward": (_i, [_vp] + [_i] * 2 + [_vp] * 5),              # stream, V N, ptr idx delta dloss dverts
    "gd_mesh_normal_consistency_forward": (_i, [_vp] + [_i] * 2 + [_vp] * 4),      # stream, F P, fn face_nbr loss scratch
    "gd_mesh_normal_consistency_backward": (_i, [_vp] + [_i] * 2 + [_vp] * 4),     # stream, F P, fn face_nbr dloss dfn
}

# the deformer's remesher: connectivity, split, collapse and flip rounds, relax, project (include/gd_mesh_remesh.h)
REMESH_FLAG_INDEX, REMESH_FLAG_REPEATED, REMESH_FLAG_NONMANIFOLD, REMESH_FLAG_CAPACITY = 0, 1, 2, 3
REMESH_FLAG_SELECTED, REMESH_FLAG_UNPROJECTED, REMESH_FLAGS = 4, 5, 8
REMESH_MAX_CELLS = 1 << 21


class RemeshMesh(C.Structure):
    """``gd_remesh_mesh``, passed by pointer"""
    _fields_ = [("V", C.c_int32), ("F", C.c_int32), ("E", C.c_int32)] + [(n, C.c_void_p) for n in (
        "verts", "tri", "ev", "eh", "bnd", "nbr_ptr", "nbr_idx", "vf_ptr", "vf_idx")]


class RemeshGrid(C.Structure):
    """``gd_remesh_grid``, passed by pointer"""
    _fields_ = [("origin", C.c_float * 3), ("cell", C.c_float), ("dims", C.c_int32 * 3)]


_RM = C.POINTER(RemeshMesh)
_RG = C.POINTER(RemeshGrid)
MESH_REMESH_SIGNATURES = {
    "gd_mesh_remesh_scan": (_i, [_vp, _i, _vp, _vp]),                              # stream, n, in out
    "gd_mesh_remesh_keys": (_i, [_vp, _i, _i] + [_vp] * 4),                        # stream, V F, tri hkeys ckeys flags
    "gd_mesh_remesh_heads": (_i, [_vp, _i] + [_vp] * 3),                           # stream, n, sorted head flags
    "gd_mesh_remesh_edge_tables": (_i, [_vp] + [_i] * 3 + [_vp] * 10),             # stream, V F E, sorted order scan fe ev eh
                                                                                   # ukeys rkeys bnd flags
    "gd_mesh_remesh_vertex_tables": (_i, [_vp] + [_i] * 3 + [_vp] * 7),            # ..., ukeys srkeys sckeys nbr_ptr nbr_idx
                                                                                   # vf_ptr vf_idx
    "gd_mesh_remesh_split_mark": (_i, [_vp, _i, _i, _vp, _vp, _f, _vp]),           # stream, V E, verts ev, hi2, mark
    "gd_mesh_remesh_split_count": (_i, [_vp, _i, _i] + [_vp] * 3),                 # stream, F E, fe mark count
    "gd_mesh_remesh_split_apply": (_i, [_vp] + [_i] * 5 + [_vp] * 10),             # stream, V F E Vcap Fcap, verts tri ev fe
                                                                                   # mark escan fscan verts_out tri_out flags
    "gd_mesh_remesh_collapse_candidates": (_i, [_vp, _RM, _f, _f] + [_vp] * 3),    # stream, mesh, lo2 hi2, dir ekey vkey
    "gd_mesh_remesh_collapse_select": (_i, [_vp, _RM] + [_vp] * 5),                # stream, mesh, dir ekey vkey remap flags
    "gd_mesh_remesh_relabel": (_i, [_vp, _i, _i] + [_vp] * 5),                     # stream, V F, tri remap tri_out alive flags
    "gd_mesh_remesh_compact_faces": (_i, [_vp, _i, _i] + [_vp] * 5),               # stream, F Fcap, tri alive scan out flags
    "gd_mesh_remesh_flip_candidates": (_i, [_vp, _RM] + [_vp] * 3),                # stream, mesh, quad ekey vkey
    "gd_mesh_remesh_flip_apply": (_i, [_vp] + [_i] * 3 + [_vp] * 6),               # stream, V F E, eh quad ekey vkey tri flags
    "gd_mesh_remesh_relax": (_i, [_vp, _RM, _vp, _vp]),                            # stream, mesh, verts_out moved
    "gd_mesh_remesh_grid_bin": (_i, [_vp, _RG, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp]),  # stream, grid, V F, verts tri,
                                                                                   # scatter, count start items, capacity, flags
    "gd_mesh_remesh_project": (_i, [_vp, _RG, _i, _vp, _vp, _i, _i] + [_vp] * 4 + [_i, _vp, _vp]),  # stream, grid, n, points
                                                              # moved, V F, verts tri start items, capacity, out flags
    "gd_mesh_remesh_used_vertices": (_i, [_vp, _i, _i] + [_vp] * 3),               # stream, V F, tri used flags
    "gd_mesh_remesh_compact_vertices": (_i, [_vp] + [_i] * 3 + [_vp] * 7),         # stream, V F Vcap, verts tri used scan
                                                                                   # verts_out tri_out flags
    "gd_mesh_remesh_edge_lengths": (_i, [_vp, _i, _i] + [_vp] * 3),                # stream, V E, verts edges len
}

# the final mesh's post-process: quadric decimation, Taubin smoothing, rotation (include/gd_mesh_simplify.h); it shares the
# connectivity, the flags and the compaction entries of the remesher
MESH_SIMPLIFY_SIGNATURES = {
    "gd_mesh_simplify_quadrics": (_i, [_vp, _RM, _vp]),                            # stream, mesh, Q
    "gd_mesh_simplify_candidates": (_i, [_vp, _RM] + [_vp] * 4),                   # stream, mesh, Q key dir cost
    "gd_mesh_simplify_spread": (_i, [_vp, _RM] + [_vp] * 4),                       # stream, mesh, key threshold lock vkey
    "gd_mesh_simplify_select": (_i, [_vp, _RM] + [_vp] * 8),                       # stream, mesh, key threshold dir vkey remap
                                                                                   # Q lock flags
    "gd_mesh_simplify_smooth": (_i, [_vp, _RM, _f, _vp]),                          # stream, mesh, w, verts_out
    "gd_mesh_simplify_rotate": (_i, [_vp, _i, _vp, _vp]),                          # stream, V, verts verts_out
}

# mesh cleaning: weld, null and duplicate faces, small components, non-manifold edges and vertices
# (include/gd_mesh_clean.h); it shares the grid struct and the scan of the remesher
CLEAN_STATS = 16
CLEAN_STAT_INDEX, CLEAN_STAT_NONFINITE, CLEAN_STAT_REFERENCED, CLEAN_STAT_MERGED, CLEAN_STAT_NULL = 0, 1, 2, 3, 4
CLEAN_STAT_DUPLICATE, CLEAN_STAT_COMPONENTS, CLEAN_STAT_COMPONENTS_REMOVED, CLEAN_STAT_COMPONENT_FACES = 5, 6, 7, 8
CLEAN_STAT_SPLIT = 9
CLEAN_MAX_ROUNDS = 16
CLEAN_MAX_CELLS = 1 << 21
MESH_CLEAN_SIGNATURES = {
    "gd_mesh_clean_check": (_i, [_vp, _i, _i] + [_vp] * 6),                        # stream, V F, verts tri used box box_keys stats
    "gd_mesh_clean_grid_bin": (_i, [_vp, _RG, _i, _vp, _vp, _i, _vp, _vp, _vp]),   # stream, grid, V, verts used, scatter, count
                                                                                   # start items
    "gd_mesh_clean_merge_rounds": (_i, [_vp, _RG, _i] + [_vp] * 4 + [_f, _i] + [_vp] * 3),   # stream, grid, V, verts used start
                                                                                   # items, r2 rounds, state_a state_b undecided
    "gd_mesh_clean_merge_target": (_i, [_vp, _RG, _i] + [_vp] * 4 + [_f, _i] + [_vp] * 3),   # ..., r2 merge, state target stats
    "gd_mesh_clean_relabel": (_i, [_vp, _i, _i] + [_vp] * 7),                      # stream, V F, verts tri target tri_out alive
                                                                                   # akey stats
    "gd_mesh_clean_edge_keys": (_i, [_vp, _i, _i] + [_vp] * 3),                    # stream, V F, tri alive hkeys
    "gd_mesh_clean_edge_table": (_i, [_vp, _i] + [_vp] * 4),                       # stream, n, skeys order she pos
    "gd_mesh_clean_duplicates": (_i, [_vp, _i] + [_vp] * 7),                       # stream, F, tri alive_in skeys she pos
                                                                                   # alive_out stats
    "gd_mesh_clean_face_sweeps": (_i, [_vp, _i] + [_vp] * 3 + [_i, _i] + [_vp] * 2),   # stream, F, skeys she alive, sweeps init,
                                                                                   # parent changed
    "gd_mesh_clean_component_stats": (_i, [_vp, _i, _i] + [_vp] * 6),              # stream, V F, verts tri alive parent ckeys
                                                                                   # ccount
    "gd_mesh_clean_component_filter": (_i, [_vp, _i] + [_vp] * 4 + [_i, _f] + [_vp] * 3),   # stream, F, alive_in parent ckeys
                                                                                   # ccount, min_faces t2, label alive_out stats
    "gd_mesh_clean_edge_rounds": (_i, [_vp, _i] + [_vp] * 3 + [_i] + [_vp] * 3),   # stream, F, skeys she akey, rounds, live_a
                                                                                   # live_b over
    "gd_mesh_clean_corner_sweeps": (_i, [_vp, _i] + [_vp] * 4 + [_i, _i] + [_vp] * 2),   # stream, F, tri skeys she alive,
                                                                                   # sweeps init, parent changed
    "gd_mesh_clean_fan_roots": (_i, [_vp, _i, _i] + [_vp] * 7),                    # stream, V F, tri alive parent vmin used
                                                                                   # split_key stats
    "gd_mesh_clean_fan_ranks": (_i, [_vp, _i, _i, _vp, _vp]),                      # stream, n S, sorted_keys crank
    "gd_mesh_clean_compact_faces": (_i, [_vp, _i, _i] + [_vp] * 5),                # stream, F Fout, tri alive fscan tri_out face_map
    "gd_mesh_clean_emit": (_i, [_vp] + [_i] * 5 + [_vp] * 14),                     # stream, V F Fout V0 S, verts tri alive fscan
                                           # used vscan target parent crank sorted_keys verts_out tri_out face_map vertex_map
}

# reading the captured views: the PNG row unfilter and the unpacking into float images (include/gd_views.h); messages go
# through gd_mesh_last_error
VIEWS_MAX_SIDE = 8192
VIEWS_SIGNATURES = {
    "gd_views_png_unfilter": (_i, [_vp, _vp, _vp] + [_i] * 4),                     # stream, filtered out, B H W bpp
    "gd_views_unpack": (_i, [_vp, _vp, _vp, _i] + [_vp] * 3 + [_i] * 2),           # stream, normal_rgba rgb, rgb_channels,
                                                                                   # normal mask rgb_out, H W
    "gd_views_unpack_rgba": (_i, [_vp] * 4 + [_i] * 2),                            # stream, rgba rgb_out mask, H W
}

# the second stage's G-buffer losses: enhanced / plain normal map and hole mask, one view per call (include/gd_mesh_losses.h)
MESH_LOSS_ENHANCED, MESH_LOSS_PLAIN, MESH_LOSS_HOLE = 1, 2, 4
MESH_LOSS_STATS_WORDS = 6
MESH_LOSS_SIGNATURES = {
    "gd_mesh_gbuffer_losses_scratch_bytes": (C.c_size_t, [C.c_int64]),
    "gd_mesh_gbuffer_losses_forward": (_i, [_vp] + [_i] * 3 + [_vp] * 9 + [_f] + [_vp] * 2),   # stream, H W terms, normal position
                                                    # mask, the same _rf, target normal / mask, camera, epsilon, stats scratch
    "gd_mesh_gbuffer_losses_backward": (_i, [_vp] + [_i] * 3 + [_vp] * 9 + [_f] + [_vp] * 4),  # ..., epsilon, stats dloss dnormal
                                                                                               # dposition
}

# the NeTF stage's texture field: hash-grid encoding and the fused albedo MLP (include/gd_texture.h)
TEXTURE_MAX_LEVELS = 16


class TextureLayout(C.Structure):
    """``gd_texture_layout``, passed by value"""
    _fields_ = [("num_levels", C.c_int32), ("scale", C.c_float * TEXTURE_MAX_LEVELS),
                ("res", C.c_int32 * TEXTURE_MAX_LEVELS), ("size", C.c_int32 * TEXTURE_MAX_LEVELS),
                ("offset", C.c_int32 * (TEXTURE_MAX_LEVELS + 1))]


TEXTURE_SIGNATURES = {
    "gd_texture_encode_forward": (_i, [_vp, _i, _vp, _vp, _vp, TextureLayout, _vp]),       # stream, N, x mask grid, layout, enc
    "gd_texture_encode_backward": (_i, [_vp, _i, _vp, _vp, _vp, TextureLayout, _vp]),      # stream, N, x mask denc, layout, dgrid
    "gd_texture_field_forward": (_i, [_vp, _i, _vp, _vp, _vp, TextureLayout] + [_vp] * 5), # ..., w1 b1 w2 b2 color
    "gd_texture_field_backward_scratch_bytes": (C.c_size_t, [_i]),
    "gd_texture_field_backward": (_i, [_vp, _i, _vp, _vp, _vp, TextureLayout] + [_vp] * 12),  # ..., w1 b1 w2 b2 color dcolor
                                                                                               # dgrid dw1 db1 dw2 db2 scratch
    "gd_texture_last_error": (C.c_char_p, []),
}

# its opt-in reproducible grid gradient: dgrid by stable sort and sum (include/gd_texture_sorted.h); messages go through
# gd_texture_last_error
TEXTURE_SORTED_MAX_POINTS = 1 << 24
TEXTURE_SORTED_SIGNATURES = {
    "gd_texture_sorted_scratch_bytes": (C.c_size_t, [_i, TextureLayout]),
    "gd_texture_encode_backward_sorted": (_i, [_vp, _i, _vp, _vp, _vp, TextureLayout, _vp, _vp]),  # ..., denc, layout, dgrid scratch
    "gd_texture_field_backward_sorted": (_i, [_vp, _i, _vp, _vp, _vp, TextureLayout] + [_vp] * 14),  # as field_backward up to
                                                                                    # db2, then denc slab_scratch sort_scratch
}

# its opt-in gradient to the sample positions (include/gd_texture_position.h); messages go through gd_texture_last_error
TEXTURE_POSITION_SIGNATURES = {
    "gd_texture_encode_backward_pos": (_i, [_vp, _i, _vp, _vp, _vp, TextureLayout, _vp, _vp]),  # stream, N, x mask grid, layout, denc dx
    "gd_texture_field_backward_pos": (_i, [_vp, _i, _vp, _vp, _vp, TextureLayout] + [_vp] * 13),  # as field_backward up to db2,
                                                                                                   # then dx scratch
    "gd_texture_field_backward_sorted_pos": (_i, [_vp, _i, _vp, _vp, _vp, TextureLayout] + [_vp] * 15),  # as ..._sorted up to
                                                                                         # denc, then dx slab_scratch sort_scratch
}

# the texture bake's padding: nearest covered texel and the 8-bit gather (include/gd_bake.h)
BAKE_MAX_PADDING = 64
BAKE_MAX_CHANNELS = 4
BAKE_SIGNATURES = {
    "gd_bake_pad_index": (_i, [_vp] + [_i] * 3 + [_vp] * 2),                       # stream, H W padding, mask src
    "gd_bake_resolve_u8": (_i, [_vp] + [_i] * 3 + [_vp] * 3),                      # stream, H W C, image src out
    "gd_bake_last_error": (C.c_char_p, []),
}

# the chart-based UV atlas of the export: classes, charts, bounds, corners, lost faces (include/gd_atlas.h); messages go
# through gd_mesh_last_error
ATLAS_DEGENERATE = 6
ATLAS_MAX_SWEEPS = 64
ATLAS_MAX_RESOLUTION = 16384
ATLAS_MAX_GUTTER = 64
ATLAS_BISECTION_STEPS = 24
ATLAS_SIGNATURES = {
    "gd_atlas_face_class": (_i, [_vp, _i, _i] + [_vp] * 3),                          # stream, V F, verts tri cls
    "gd_atlas_hook": (_i, [_vp, _i, _i] + [_vp] * 6),                                # stream, F E, eh cls layer single parent
                                                                                     # changed
    "gd_atlas_jump": (_i, [_vp, _i, _vp]),                                           # stream, F, parent
    "gd_atlas_roots": (_i, [_vp, _i] + [_vp] * 3),                                   # stream, F, cls parent is_root
    "gd_atlas_bounds": (_i, [_vp] + [_i] * 3 + [_vp] * 9),                           # stream, V F C, verts tri cls parent scan
                                                                                     # face_chart keys bounds count
    "gd_atlas_emit": (_i, [_vp] + [_i] * 5 + [_f] + [_vp] * 8),                      # stream, V F C resolution gutter, scale,
                                                             # verts tri cls face_chart bounds offsets corner_xy key
    "gd_atlas_write_vt": (_i, [_vp] + [_i] * 3 + [_vp] * 4),                         # stream, n T resolution, row corner_xy vt ft
    "gd_atlas_lost_faces": (_i, [_vp] + [_i] * 3 + [_vp] * 2 + [_i] + [_vp] * 3),    # stream, F H W, corner_xy rast, freeze,
                                                                                     # lost layer single
}

# texture sampling for the textured render: rast_db, attribute derivatives, mip pyramid, the filter modes and the gradient
# to the texture (include/gd_sample.h); messages go through gd_mesh_last_error
SAMPLE_MAX_SIDE = 16384
SAMPLE_MAX_LEVELS = 15
SAMPLE_MAX_CHANNELS = 4
SAMPLE_TEXEL = 4
SAMPLE_FILTERS = {"nearest": 0, "linear": 1, "linear-mipmap-nearest": 2, "linear-mipmap-linear": 3}
SAMPLE_BOUNDARIES = {"wrap": 0, "clamp": 1}


class SamplePyramid(C.Structure):
    """``gd_sample_pyramid``, passed by value"""
    _fields_ = [("levels", C.c_int32), ("width", C.c_int32 * SAMPLE_MAX_LEVELS), ("height", C.c_int32 * SAMPLE_MAX_LEVELS),
                ("offset", C.c_int32 * (SAMPLE_MAX_LEVELS + 1))]


SAMPLE_SIGNATURES = {
    "gd_sample_pyramid_layout": (_i, [_i] * 3 + [C.POINTER(SamplePyramid)]),         # Ht Wt max_mip_level, out
    "gd_sample_taps": (_i, [_i]),
    "gd_sample_rast_db": (_i, [_vp] + [_i] * 4 + [_vp] * 4),                         # stream, V F H W, rast pos tri rast_db
    "gd_sample_interpolate_da": (_i, [_vp] + [_i] * 5 + [_vp] * 5),                  # stream, V F C H W, attr rast rast_db tri
                                                                                     # out_da
    "gd_sample_build_mips": (_i, [_vp, _i, _vp, SamplePyramid, _vp]),                # stream, C, tex, layout, pyr
    "gd_sample_texture_forward": (_i, [_vp] + [_i] * 4 + [SamplePyramid] + [_vp] * 4),   # stream, N C filter boundary, layout,
                                                                                     # pyr uv uv_da out
    "gd_sample_texture_items": (_i, [_vp] + [_i] * 4 + [SamplePyramid] + [_vp] * 5), # ..., layout, uv uv_da dout keys vals
    "gd_sample_texture_reduce": (_i, [_vp, C.c_int64, _i, SamplePyramid] + [_vp] * 4),   # stream, items C, layout, sorted_keys
                                                                                     # order vals gpyr
    "gd_sample_texture_fold": (_i, [_vp, _i, SamplePyramid, _vp, _vp]),              # stream, C, layout, gpyr dtex
}

# the second stage's neural shader and shading loss (include/gd_shader.h, which also fixes the layouts of the buffers);
# messages go through gd_mesh_last_error
_u32 = C.c_uint32
_i64 = C.c_int64
SHADER_LAYERS = 8
SHADER_TILE_ROWS = 128
SHADER_PACKED_ELEMS = 327680
SHADER_PARAM_ELEMS = 320960
SHADER_SIGNATURES = {
    "gd_shader_select_scratch_bytes": (C.c_size_t, [_i64]),
    "gd_shader_scratch_bytes": (C.c_size_t, [_i64]),
    "gd_shader_select": (_i, [_vp, _i, _i] + [_vp] * 5 + [_f, _u32, _u32, _i64] + [_vp] * 3),  # stream, H W, normal position
                                                     # mask view_mask camera, p seed step capacity, index counters scratch
    "gd_shader_features": (_i, [_vp, _i, _i] + [_vp] * 3 + [_i64] + [_vp] * 3),     # ..., position normal camera, capacity,
                                                                                     # index counters act
    "gd_shader_features_points": (_i, [_vp, _i64] + [_vp] * 3 + [_i64] + [_vp] * 2),  # stream, N, position normal view_dir,
                                                                                     # capacity, counters act
    "gd_shader_pack": (_i, [_vp] * 4),                                               # stream, params packed packed_t
    "gd_shader_forward_layer": (_i, [_vp, _i, _i64] + [_vp] * 5),                    # stream, l capacity, counters packed
                                                                                     # params act logits
    "gd_shader_backward_input_layer": (_i, [_vp, _i, _i64] + [_vp] * 6),             # ..., counters packed_t act dz dfeat dextra
    "gd_shader_backward_weight_layer": (_i, [_vp, _i, _i64] + [_vp] * 5),            # ..., counters act dz grad scratch
    "gd_shader_l1_forward": (_i, [_vp, _i, _i, _i64] + [_vp] * 6),                   # stream, H W capacity, index counters
                                                                                     # logits rgb loss scratch
    "gd_shader_l1_backward": (_i, [_vp, _i, _i, _i64] + [_vp] * 7),                  # ..., logits rgb dloss dz dlogits
    "gd_shader_colour": (_i, [_vp, _i64, _vp, _vp]),                                 # stream, N, logits colour
    "gd_shader_features_backward": (_i, [_vp, _i, _i] + [_vp] * 2 + [_i64] + [_vp] * 6),  # stream, H W, position camera,
                                                                    # capacity, index counters dfeat dextra dposition dnormal
}

# the loss head of the NeTF stage's texture fit (include/gd_fit.h); messages go through gd_mesh_last_error
FIT_PIXELS_PER_LANE = 4
FIT_PIXELS_PER_PARTIAL = 256
FIT_FINAL_THREADS = 256
FIT_STATS_WORDS = 4
FIT_SIGNATURES = {
    "gd_fit_loss_scratch_bytes": (C.c_size_t, [_i64]),
    "gd_fit_loss_forward": (_i, [_vp] + [_i] * 3 + [_vp] * 13),                      # stream, H W flip_rows, c_aa a_aa p_aa n_aa
                                                                 # center rgb tmask bg, image cosinesview m stats scratch
    "gd_fit_loss_backward": (_i, [_vp] + [_i] * 3 + [_vp] * 8),                      # ..., c_aa a_aa rgb bg m stats dloss dc_aa
}


class NativeLibraryError(RuntimeError):
    pass


def lib_path() -> str:
    return _LIB_PATH


def lib():
    """Load libgd_raster.so (once).  Raises NativeLibraryError if it is absent -- no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise NativeLibraryError(
                f"{_LIB_PATH} not found: build it with `python -m garmentdreamer_amd._build` "
                "(hipcc --offload-arch=gfx950). The HIP rasterizer has no CPU fallback.")
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64; load it FIRST so
        # our library's DT_NEEDED libamdhip64.so.7 binds to the same instance (streams and device
        # pointers are shared with torch).  Loading ours first puts a second runtime in the
        # process and every call then fails with "no ROCm-capable device is detected".
        import torch  # noqa: F401
        try:
            L = C.CDLL(_LIB_PATH)
        except OSError as e:  # e.g. libamdhip64 missing
            raise NativeLibraryError(f"cannot load {_LIB_PATH}: {e}") from e
        for name, (res, args) in list(SIGNATURES.items()) + list(SCENE_SIGNATURES.items()) + list(MESH_SIGNATURES.items()) \
                + list(MESH_DEFORM_SIGNATURES.items()) + list(MESH_GEOMETRY_SIGNATURES.items()) \
                + list(MESH_REMESH_SIGNATURES.items()) + list(MESH_SIMPLIFY_SIGNATURES.items()) \
                + list(MESH_LOSS_SIGNATURES.items()) + list(TEXTURE_SIGNATURES.items()) + list(TEXTURE_SORTED_SIGNATURES.items()) \
                + list(TEXTURE_POSITION_SIGNATURES.items()) \
                + list(BAKE_SIGNATURES.items()) + list(SHADER_SIGNATURES.items()) + list(FIT_SIGNATURES.items()) \
                + list(ATLAS_SIGNATURES.items()) + list(SAMPLE_SIGNATURES.items()) + list(MESH_CLEAN_SIGNATURES.items()) \
                + list(VIEWS_SIGNATURES.items()):
            fn = getattr(L, name)  # AttributeError here == ABI drift; let it surface
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


# prefix of an entry's name -> the symbol that holds its message, longest prefix first (gd_scene_densify_stats lives in
# raster_scene.hip with the scene entries; plan and apply in raster_densify.hip have a channel of their own)
_ERROR_CHANNELS = (("gd_scene_densify_stats", "gd_scene_last_error"), ("gd_scene_densify_", "gd_scene_densify_last_error"),
                   ("gd_scene_", "gd_scene_last_error"), ("gd_mesh_", "gd_mesh_last_error"),
                   ("gd_shader_", "gd_mesh_last_error"), ("gd_fit_", "gd_mesh_last_error"),
                   ("gd_atlas_", "gd_mesh_last_error"), ("gd_sample_", "gd_mesh_last_error"),
                   ("gd_views_", "gd_mesh_last_error"),
                   ("gd_texture_", "gd_texture_last_error"), ("gd_bake_", "gd_bake_last_error"),
                   ("gd_raster_", "gd_raster_last_error"))


def error_channel(name: str) -> str:
    """The ``gd_*_last_error`` symbol that holds the message of a failed ``name``: the one of its longest prefix."""
    for prefix, channel in _ERROR_CHANNELS:
        if name.startswith(prefix):
            return channel
    raise KeyError(f"{name} belongs to no error channel of libgd_raster.so")


def checked(name: str, ret: int, channel: Optional[str] = None) -> int:
    """``ret`` of the entry ``name`` if it is not negative; else ``RuntimeError`` with the text of its error channel."""
    if ret < 0:
        text = getattr(lib(), channel or error_channel(name))().decode("utf-8", "replace")
        raise RuntimeError(f"{name} failed ({ret}): {text}")
    return ret


def check(ret: int, what: str) -> int:
    return ret if ret >= 0 else checked(what, ret, "gd_raster_last_error")


def check_scene(ret: int, what: str, err: str = "gd_scene_last_error") -> int:
    return ret if ret >= 0 else checked(what, ret, err)


KERNEL_IDS = {"preprocess": 0, "scan": 1, "duplicate": 2, "sort": 3, "ranges": 4, "render_fwd": 5, "render_bwd": 6,
              "preprocess_bwd": 7}


def profile_enable(on: bool) -> None:
    lib().gd_raster_profile_enable(int(on))


def profile_reset() -> None:
    lib().gd_raster_profile_reset()


def profile_read() -> dict:
    """{kernel: (total_ms, launches)} after waiting for all recorded events."""
    L = lib()
    L.gd_raster_profile_collect()
    out = {}
    for name, kid in KERNEL_IDS.items():
        ms, n = C.c_double(0), C.c_int64(0)
        L.gd_raster_profile_get(kid, C.byref(ms), C.byref(n))
        out[name] = (ms.value, n.value)
    return out
