"""ctypes binding of liborip.so (include/orip.h).  Fails loudly when the HIP library is missing: the
product has no CPU path (the CPU restatement under oracle/ is test infrastructure and is never imported here)."""
from __future__ import annotations

import ctypes as C
import os

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_PKG, "liborip.so")

# One hardware queue per lane (layer pipelines, raster stages, stage 10): HIP multiplexes its streams onto GPU_MAX_HW_QUEUES
# (default 4) hardware queues and kernels sharing a queue run one after the other, so a short kernel of one layer would wait
# behind a long walk of another.  Must be in the environment before the HIP runtime initialises (bench.py sets it before torch).
# This line only fills an unset variable, for a host that starts HIP (torch) between this import and its first Device.  The request that
# always holds is the library's own: the first orip_create of the process overrides a value below 16 that a launcher set (such a default
# costs a third of the step: 122 against 74 ms at 4096^2 x 8) and keeps one from 16 to 32; it only takes effect when that call is the
# process's first HIP call (a host that initialised HIP earlier keeps what it had).  orip_hw_queues reports what it found and left.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

MAX_LAYERS = 16
SLOT_CONTOURS, SLOT_SCALED, SLOT_SORTED, SLOT_LINES_INTRA, SLOT_LINES_CROSS = range(5)
TAPS_INTRA, TAPS_CROSS = 0, 1


class Params08(C.Structure):
    _fields_ = [("tap_diam", C.c_double), ("tap_max_dim", C.c_double), ("min_keep", C.c_double), ("tap_max_per", C.c_double),
                ("tap_max_v", C.c_int32), ("sample_step", C.c_double), ("tail_len_px", C.c_double), ("col_rad", C.c_double),
                ("grid_stride", C.c_double), ("max_jump", C.c_double), ("post_on", C.c_int32), ("post_brush", C.c_int32),
                ("post_step", C.c_double), ("post_eps", C.c_double), ("post_minlen", C.c_int32), ("W", C.c_int32), ("H", C.c_int32),
                ("brush_forbid", C.c_int32)]


class Params10(C.Structure):
    _fields_ = [("tap_diam", C.c_double), ("min_keep", C.c_double), ("tap_max_per", C.c_double), ("tap_max_v", C.c_int32),
                ("max_jump", C.c_double), ("D_lines", C.c_double), ("D_taps", C.c_double), ("step_px", C.c_double),
                ("W", C.c_int32), ("H", C.c_int32)]


class GcodeMap(C.Structure):
    _fields_ = [("scale_x", C.c_double), ("scale_y", C.c_double), ("offset_x_mm", C.c_double), ("offset_y_mm", C.c_double), ("steps_per_mm", C.c_double),
                ("W", C.c_int32), ("H", C.c_int32), ("invert_y", C.c_int32)]


_vp, _i64, _i32, _f64, _f32, _cp = C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_float, C.c_char_p
_P = C.POINTER

# name -> (restype, argtypes); every symbol include/orip.h declares
SIGNATURES = {
    "orip_create": (_i32, [_i32, _P(_vp)]), "orip_destroy": (None, [_vp]), "orip_hw_queues": (None, [_P(_i32), _P(_i32)]), "orip_last_error": (_cp, [_vp]), "orip_sync": (_i32, [_vp]),
    "orip_prof_reset": (_i32, [_vp]), "orip_prof_get": (_i32, [_vp, _cp, _P(_f64), _P(_i64)]), "orip_prof_enable": (_i32, [_vp, _i32]),
    "orip_resize_area": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32]),
    "orip_set_image": (_i32, [_vp, _vp, _i32, _i32]), "orip_lab_of": (_i32, [_vp, _vp, _i64, _vp]),
    "orip_kmeans_fit": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _f64, _vp, _P(_f64)]),
    "orip_kmeans_samples": (_i32, [_vp, _vp, _i64]), "orip_kmeans_samples_info": (_i32, [_vp, _P(_i64), _P(_i64)]),
    "orip_kmeans_fit_rgb": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _f64, _vp, _P(_f64)]), "orip_assign_palette": (_i32, [_vp, _vp, _i32, _vp, _vp]),
    "orip_colors_table": (_i32, [_vp, _i32, _i32, _i64, _P(_i64), _P(_i64), _P(_i32)]), "orip_colors_fetch": (_i32, [_vp, _vp, _vp, _P(_i64)]),
    "orip_colors_hue": (_i32, [_vp, _vp]), "orip_colors_kmeans": (_i32, [_vp, _i32, _i32, _i32, C.c_uint64, _vp, _vp, _vp, _vp]),
    "orip_lab_of_rgb": (_i32, [_vp, _vp, _i64, _vp]),
    "orip_extract_layers": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _vp]),
    "orip_get_labels": (_i32, [_vp, _vp]), "orip_get_mask": (_i32, [_vp, _i32, _vp]), "orip_set_masks": (_i32, [_vp, _vp, _i32, _i32, _i32]),
    "orip_keep_layers": (_i32, [_vp, _vp, _i32]),
    "orip_detect_edges": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _i32]),
    "orip_get_edges": (_i32, [_vp, _i32, _vp]), "orip_set_edges": (_i32, [_vp, _vp, _i32, _i32, _i32]),
    "orip_find_contours": (_i32, [_vp]), "orip_contours_prepare": (_i32, [_vp]), "orip_contours_reserve": (_i32, [_vp, _i32]), "orip_contours_layer": (_i32, [_vp, _i32]),
    "orip_dedup_cross_begin": (_i32, [_vp, _P(Params10)]), "orip_dedup_cross_layer": (_i32, [_vp, _i32]), "orip_dedup_cross_layer_from": (_i32, [_vp, _i32, _i32]), "orip_dedup_cross_layer_deferred": (_i32, [_vp, _i32, _i32]), "orip_get_skeleton": (_i32, [_vp, _i32, _vp]),
    "orip_polys_size": (_i32, [_vp, _i32, _i32, _P(_i64), _P(_i64)]), "orip_get_polys": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "orip_set_polys": (_i32, [_vp, _i32, _i32, _i64, _vp, _vp]),
    "orip_taps_size": (_i32, [_vp, _i32, _i32, _P(_i64)]), "orip_get_taps": (_i32, [_vp, _i32, _i32, _vp]),
    "orip_set_taps": (_i32, [_vp, _i32, _i32, _i64, _vp]), "orip_set_layer_count": (_i32, [_vp, _i32]),
    "orip_scale_vectors": (_i32, [_vp, _i32, _f32, _f32, _f32, _f32]), "orip_sort_contours": (_i32, [_vp, _i32]),
    "orip_dedup_layer": (_i32, [_vp, _i32, _P(Params08)]), "orip_layer_front": (_i32, [_vp, _i32, _f32, _f32, _f32, _f32, _i32, _vp]), "orip_dedup_cross": (_i32, [_vp, _vp, _i32, _P(Params10)]),
    "orip_plot_order": (_i32, [_vp, _i32, _f64, _P(_i64)]), "orip_get_ops": (_i32, [_vp, _i32, _vp]),
    "orip_preview_cover": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "orip_stream_codes": (_i32, [_vp, _vp, _i64, _P(_i64)]), "orip_stream_codes_fetch": (_i32, [_vp, _vp, _vp]),
    "orip_stream_preview": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp]), "orip_stream_preview_fetch": (_i32, [_vp, _vp]),
    "orip_gcode_to_steps": (_i32, [_vp, _vp, _vp, _i64, _P(GcodeMap), _P(_i64), _P(_i64)]), "orip_gcode_steps_fetch": (_i32, [_vp, _vp, _vp]),
    "orip_gcode_order": (_i32, [_vp, _vp, _i64, _vp]), "orip_gcode_steps_source_fetch": (_i32, [_vp, _vp]),
    "orip_gcode_to_steps_clip": (_i32, [_vp, _vp, _vp, _i64, _P(GcodeMap), _vp, _P(_i64), _P(_i64), _vp]),
    "orip_gcode_order_pens": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp]),
    "orip_gcode_merge": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp]), "orip_gcode_merge_fetch": (_i32, [_vp, _vp, _vp, _vp]),
    "orip_gcode_simplify": (_i32, [_vp, _vp, _vp, _i64, _i32, _vp]), "orip_gcode_simplify_fetch": (_i32, [_vp, _vp]),
    "orip_gcode_dedup": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _vp]), "orip_gcode_dedup_fetch": (_i32, [_vp, _vp]),
    "orip_gcode_occlude": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp]), "orip_gcode_occlude_fetch": (_i32, [_vp, _vp]),
    "orip_svg_occlude": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, _P(GcodeMap), _i32, _vp]),
    "orip_gcode_hatch_link": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i32, _vp]), "orip_gcode_hatch_link_fetch": (_i32, [_vp, _vp, _vp]),
    "orip_svg_hatch_link": (_i32, [_vp, _vp, _i64, _vp, _vp, _i64, _P(GcodeMap), _i32, _i32, _vp]),
    "orip_gcode_stipple": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _i32, _vp]), "orip_gcode_stipple_fetch": (_i32, [_vp, _vp, _vp]),
    "orip_svg_stipple": (_i32, [_vp, _vp, _vp, _i64, _P(GcodeMap), _i32, _i32, _i32, _i32, _vp, _i32, _vp]),
    "orip_fill_mask": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]), "orip_fill_fetch": (_i32, [_vp, _vp]),
    "orip_fill_link": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]), "orip_fill_link_fetch": (_i32, [_vp, _vp, _vp]),
    "orip_fill_stipple": (_i32, [_vp, _vp, _i32, _vp] + [_i32] * 16 + [_vp]), "orip_fill_stipple_fetch": (_i32, [_vp, _vp]),
    "orip_gcode_dash": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i32, _vp]), "orip_gcode_dash_fetch": (_i32, [_vp, _vp]),
    "orip_gcode_improve": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _i64, _vp, _vp, _vp]),
    "orip_gcode_seam": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "orip_gcode_order_rings": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "orip_svg_flatten": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _f64, _P(_i64)]), "orip_svg_paths_fetch": (_i32, [_vp, _vp, _vp]),
    "orip_svg_bbox": (_i32, [_vp, _vp]), "orip_svg_fit": (_i32, [_vp, _f64, _f64, _f64, _f64]),
    "orip_gcode_flatten": (_i32, [_vp, _vp, _vp, _i64, _vp, _i64, _f64, _P(_i64), _vp]),
    "orip_svg_hatch": (_i32, [_vp, _vp, _i64, _f64, _i32, _i32, _i32, _vp]), "orip_svg_hatch_groups_fetch": (_i32, [_vp, _vp]),
    "orip_svg_hatch_angle": (_i32, [_vp, _vp, _i64, _f64, _i32, _i32, _i32, _i32, _i32, _vp]),
    "orip_stream_pack": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64]), "orip_stream_pack_fetch": (_i32, [_vp, _vp]),
    "orip_comm_unique_id": (_i32, [_vp]), "orip_comm_init": (_i32, [_vp, _vp, _i32, _i32]), "orip_comm_destroy": (_i32, [_vp]),
    "orip_bcast_layer": (_i32, [_vp, _i32, _i32]),
}
COMM_ID_BYTES = 128
HATCH_SERPENTINE, HATCH_HORIZONTAL, HATCH_VERTICAL = 1, 2, 4
HATCH_STATS = ("groups", "lines", "crossings", "segments")
HATCH_ANGLE_STATS = HATCH_STATS + ("collapsed",)
ORDER_REVERSE, ORDER_MAX_GROUPS = 1, 64
MERGE_REVERSE = 1
SIMPLIFY_TOL4_MAX, SIMPLIFY_LOCAL = (1 << 17) - 1, 1024      # include/orip.h: the largest tolerance in quarter steps; the points one wave finishes alone
CLIP_STATS = ("segments", "inside", "cut", "outside", "paths_out", "points_out")
DEDUP_STATS = ("segments", "whole", "cut", "covered", "pieces", "paths_out", "points_out", "draw_steps_in", "draw_steps_out")
OCCLUDE_STATS = ("segments", "whole", "cut", "hidden", "pieces", "collapsed", "paths_out", "points_out", "draw_steps_in", "draw_steps_out")
OCCLUDE_CLAMP = 1
HATCH_LINK_STATS = ("lines", "in_reach", "eligible", "links", "coincident", "paths_out", "points_out", "link_steps")
HATCH_LINK_CLAMP, HATCH_LINK_REACH_MAX = 1, 1 << 20            # include/orip.h: the rings are clamped to the sheet; the longest link in steps
STIPPLE_STATS = ("groups", "rows", "candidates", "near", "outside", "hidden", "dots")
STIPPLE_SERPENTINE, STIPPLE_OCCLUDE, STIPPLE_CLAMP, STIPPLE_MAX = 1, 2, 4, 1 << 20      # include/orip.h: the flags; the largest pitch, row and inset in steps
FILL_STATS = ("lines", "samples", "on", "runs", "short", "segments")
FILL_SERPENTINE, FILL_ALONG, FILL_ACROSS = 1, 2, 4                                       # include/orip.h: the flags of orip_fill_mask
FILL_COORD_MAX, FILL_U_MAX, FILL_LEN_MAX = 1 << 20, 4096, 1 << 15                          # the largest side and offset; direction component; spacing, inset and min_len in pixels
FILL_LINK_STATS = ("segments", "in_reach", "eligible", "links", "paths_out", "points_out", "link_steps")
FILL_LINK_REACH_MAX = 1 << 15                                                             # include/orip.h: the largest reach of orip_fill_link, in pixels
FILL_STIPPLE_STATS = ("candidates", "ink", "near", "light", "dots")
FILL_STIPPLE_SERPENTINE, FILL_STIPPLE_RAD_MAX = 1, 32                                     # include/orip.h: the flag of orip_fill_stipple; the largest clear_rad and tone_rad, in source pixels
DASH_STATS = ("paths_in", "dashed", "dashes", "collapsed", "paths_out", "points_out", "length_in", "length_on")
DASH_UNIT, DASH_MAX_ENTRIES = 256, 64                        # include/orip.h: dash lengths are in 1/256 step; entries of one pattern at most
IMPROVE_MAX_PATHS, IMPROVE_ROUNDS_AUTO = 65536, (1 << 63) - 1
SEAM_STATS = ("closed", "moved", "travel_before", "travel_after")
RING_ENTRY_STATS = ("closed", "moved", "candidates", "travel")
ARC_STATS = ("arcs", "pieces", "full_circles")
ARC_LINE, ARC_CW, ARC_CCW, ARC_MAX_DEPTH = 1, 2, 3, 16         # include/orip.h: the kinds of orip_gcode_flatten; ORIP_ARC_MAX_DEPTH

_lib = None


def load():
    """Load liborip.so and declare every entry point.  Raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"liborip.so not found at {LIB_PATH}: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)   # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib
