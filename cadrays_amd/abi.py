"""ctypes mirror of include/cadrays_hip.h (the C ABI of libcadrays_hip.so).

The struct layouts are the boundary's input contract; the CPU oracle takes the same structs,
so tests hand identical bytes to both sides.
"""
import ctypes as C

OK, E_INVALID, E_DEVICE, E_NOMEM, E_NOTBUILT = 0, -1, -2, -3, -4

FRESNEL_CONSTANT, FRESNEL_CONDUCTOR, FRESNEL_DIELECTRIC = -1.0, -2.0, -3.0


class crh_bsdf(C.Structure):
    _fields_ = [(n, C.c_float * 4) for n in
                ("Kc", "Kd", "Ks", "Kt", "Le", "Absorption", "FresnelCoat", "FresnelBase")]


class crh_light(C.Structure):
    _fields_ = [("vec", C.c_float * 3), ("is_point", C.c_float),
                ("emission", C.c_float * 3), ("smoothness", C.c_float)]


class crh_camera(C.Structure):
    _fields_ = [("eye", C.c_float * 3), ("dir", C.c_float * 3), ("up", C.c_float * 3),
                ("fovy_deg", C.c_float), ("aspect", C.c_float), ("is_ortho", C.c_int32),
                ("ortho_scale", C.c_float), ("aperture_radius", C.c_float), ("focal_dist", C.c_float)]


class crh_params(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("max_depth", C.c_uint32),
                ("radiance_clamp", C.c_float), ("two_sided", C.c_int32), ("coherent_rng", C.c_int32),
                ("seed", C.c_uint32), ("tile_size", C.c_uint32), ("tonemap_mode", C.c_int32),
                ("exposure", C.c_float), ("white_point", C.c_float), ("background", C.c_float * 3),
                ("env_as_background", C.c_int32), ("scene_epsilon", C.c_float),
                ("russian_roulette", C.c_int32)]


class crh_stats(C.Structure):
    _fields_ = [("rays_nearest", C.c_uint64), ("rays_any", C.c_uint64), ("nodes_nearest", C.c_uint64),
                ("tris_nearest", C.c_uint64), ("nodes_any", C.c_uint64), ("tris_any", C.c_uint64), ("shaded_hits", C.c_uint64), ("samples", C.c_uint64),
                ("seconds", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class crh_spec(C.Structure):
    """include/crh_spec.h: the switchable departures from the recollected OCCT behaviour; defaults = the frozen spec"""
    _fields_ = [("size", C.c_uint32), ("uniform_32bit", C.c_int32), ("texel_gamma2", C.c_int32), ("mis_single_lobe", C.c_int32),
                ("eps_rule", C.c_int32), ("eta_no_dielectric", C.c_float),
                ("rr_start_bounce", C.c_int32), ("rr_survival_cap", C.c_float), ("min_contribution", C.c_float), ("min_throughput", C.c_float),
                ("raygen_bilinear", C.c_int32), ("env_orientation", C.c_int32), ("display_gamma22", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "size"}


class crh_pick_result(C.Structure):
    """what crh_pick reports for one pixel (include/cadrays_hip.h)"""
    _fields_ = [("object", C.c_int32), ("triangle", C.c_int32), ("t", C.c_float), ("depth", C.c_float), ("u", C.c_float), ("v", C.c_float),
                ("point", C.c_float * 3)]

    def as_dict(self):
        return {"object": int(self.object), "triangle": int(self.triangle), "t": self.t, "depth": self.depth, "u": self.u, "v": self.v,
                "point": tuple(self.point)}


class crh_meter_params(C.Structure):
    """the metering rule's parameters (include/cadrays_hip.h; crh_meter_defaults fills them: METER_DEFAULTS below)"""
    _fields_ = [("key_stops", C.c_float), ("min_stops", C.c_float), ("max_stops", C.c_float), ("white_permille", C.c_uint32),
                ("white_min", C.c_float), ("white_max", C.c_float), ("rect", C.c_uint32 * 4)]


class crh_meter_result(C.Structure):
    """what crh_measure_exposure reports (include/cadrays_hip.h)"""
    _fields_ = [("hist", C.c_uint32 * 256), ("n_unsampled", C.c_uint32), ("n_lit", C.c_uint32), ("exposure", C.c_float), ("white_point", C.c_float),
                ("white_bin", C.c_uint32)]


class crh_fit_result(C.Structure):
    """what crh_fit_view / crh_fit_from_extents report (include/cadrays_hip.h)"""
    _fields_ = [("extents", C.c_float * 6), ("right", C.c_float * 3), ("up", C.c_float * 3), ("fwd", C.c_float * 3), ("kx", C.c_float), ("ky", C.c_float),
                ("z_near", C.c_float), ("z_far", C.c_float), ("n_vertices", C.c_uint32), ("binding", C.c_int32)]

    def as_dict(self):
        import numpy as np
        d = {n: np.array(getattr(self, n), np.float32) for n in ("extents", "right", "up", "fwd")}
        d.update({n: np.float32(getattr(self, n)) for n in ("kx", "ky", "z_near", "z_far")})
        d.update(n_vertices=int(self.n_vertices), binding=int(self.binding))
        return d


class crh_region_stats(C.Structure):
    """one record of crh_query_region / crh_region_stats_host (include/cadrays_hip.h): an object's (or the background's) pixels inside the region and in the frame,
    the half-open screen box and the depth range of the pixels inside"""
    _fields_ = [("pixels", C.c_uint32), ("pixels_frame", C.c_uint32), ("x0", C.c_uint32), ("y0", C.c_uint32), ("x1", C.c_uint32), ("y1", C.c_uint32),
                ("t_min", C.c_float), ("t_max", C.c_float)]


REGION_TOUCHED, REGION_ENCLOSED = 0, 1      # crh_region_select
REGION_STATS_DTYPE = [("pixels", "<u4"), ("pixels_frame", "<u4"), ("x0", "<u4"), ("y0", "<u4"), ("x1", "<u4"), ("y1", "<u4"), ("t_min", "<f4"), ("t_max", "<f4")]   # numpy view of the records

class crh_outline_params(C.Structure):
    """the feature lines' parameters (include/cadrays_hip.h; crh_outline_defaults fills them: OUTLINE_DEFAULTS below)"""
    _fields_ = [("kinds", C.c_uint32), ("crease_cos", C.c_float), ("depth_ratio", C.c_float), ("width", C.c_uint32), ("rgb", C.c_uint8 * 3), ("alpha", C.c_uint8)]


OUTLINE_OBJECT, OUTLINE_DEPTH, OUTLINE_CREASE = 1, 2, 4      # crh_outline_params.kinds, the bits of crh_read_outline's mask
OUTLINE_ALL = OUTLINE_OBJECT | OUTLINE_DEPTH | OUTLINE_CREASE
OUTLINE_TABLE_DTYPE = [("n", "<f4", (3,)), ("degenerate", "<u4"), ("v", "<u4", (3,)), ("pad", "<u4")]      # numpy view of the per-triangle table (32 B)

class crh_denoise_params(C.Structure):
    """the denoised display's parameters (include/cadrays_hip.h; crh_denoise_defaults fills them: DENOISE_DEFAULTS below)"""
    _fields_ = [("levels", C.c_uint32), ("normal_cos", C.c_float), ("depth_ratio", C.c_float), ("until_samples", C.c_uint32)]


class crh_shade_guide_params(C.Structure):
    """the shade guide's parameters (include/cadrays_hip.h; crh_shade_guide_defaults fills them: SHADE_GUIDE_DEFAULTS below)"""
    _fields_ = [("demodulate", C.c_uint32), ("lights", C.c_uint32), ("albedo_floor", C.c_float), ("light_dilate", C.c_uint32)]


class crh_shade_guide_scene(C.Structure):
    """what crh_shade_guide_host reads of a scene (include/cadrays_hip.h)"""
    _fields_ = [("mats", C.POINTER(crh_bsdf)), ("texels", C.POINTER(C.c_float)), ("tex_desc", C.POINTER(C.c_uint32)), ("lights", C.POINTER(crh_light)),
                ("n_mats", C.c_uint32), ("n_texels", C.c_uint32), ("n_tex", C.c_uint32), ("n_lights", C.c_uint32), ("gamma2", C.c_int32)]


GUIDE_TABLE_DTYPE = [("uv", "<f4", (3, 2)), ("material", "<i4"), ("has_uv", "<u4")]      # numpy view of the shade guide's per-triangle table (32 B)


class crh_reproject_params(C.Structure):
    """the reprojected display history's parameters (include/cadrays_hip.h; crh_reproject_defaults fills them: REPROJECT_DEFAULTS below)"""
    _fields_ = [("max_history", C.c_float), ("until_samples", C.c_uint32), ("normal_cos", C.c_float), ("depth_ratio", C.c_float)]


class crh_reproject_frame(C.Structure):
    """the camera frame of the view a display history was taken from (include/cadrays_hip.h; crh_reproject_frame_host derives it from a camera)"""
    _fields_ = [("eye", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3), ("fwd", C.c_float * 3), ("tan_half", C.c_float), ("aspect", C.c_float),
                ("ortho_scale", C.c_float), ("is_ortho", C.c_uint32)]


class crh_reproject_motion_params(C.Structure):
    """the per-object history deltas' caps (include/cadrays_hip.h; crh_reproject_motion_defaults fills them: REPROJECT_MOTION_DEFAULTS below)"""
    _fields_ = [("max_history_moved", C.c_float), ("max_history_static", C.c_float)]


REPROJECT_DELTA_DTYPE = [("D", "<f4", (12,)), ("flag", "<u4"), ("pad", "<u4", (3,))]      # numpy view of the delta table's records (crh_reproject_delta, 64 B)


class crh_view_params(C.Structure):
    """the viewport read-out's parameters (include/cadrays_hip.h; all zero but the size = the whole frame, CRH_VIEW_AUTO: VIEW_DEFAULTS below)"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("src", C.c_uint32 * 4), ("filter", C.c_uint32), ("reserved", C.c_uint32)]


VIEW_AUTO, VIEW_NEAREST, VIEW_BILINEAR, VIEW_AREA = 0, 1, 2, 3      # crh_view_params.filter
VIEW_MAX_SIDE = 8192

class crh_annot_segment(C.Structure):
    """one annotation segment (include/cadrays_hip.h): world-space end points, colour, alpha, style = width (bits 0-3) | mode << 8"""
    _fields_ = [("a", C.c_float * 3), ("b", C.c_float * 3), ("rgb", C.c_uint8 * 3), ("alpha", C.c_uint8), ("style", C.c_uint32)]


class crh_annot_params(C.Structure):
    """the annotations' parameters (include/cadrays_hip.h; crh_annot_defaults fills them: ANNOT_DEFAULTS below)"""
    _fields_ = [("depth_bias", C.c_float), ("hidden_alpha", C.c_uint32)]


ANNOT_ON_TOP, ANNOT_HIDE, ANNOT_XRAY = 0, 1, 2      # the mode in bits 8-9 of crh_annot_segment.style
ANNOT_MAX_SEGMENTS = 65536
ANNOT_SEGMENT_DTYPE = [("a", "<f4", (3,)), ("b", "<f4", (3,)), ("rgb", "u1", (3,)), ("alpha", "u1"), ("style", "<u4")]      # numpy view of the list (32 B)
ANNOT_RECORD_DTYPE = [("x0", "<f4"), ("y0", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("q0", "<f4"), ("q1", "<f4"), ("flags", "<u4"), ("pad", "<u4")]      # ... of the screen records (32 B)


def annot_style(width=1, mode=ANNOT_ON_TOP):
    """CRH_ANNOT_STYLE: the style word of a segment `width` pixels wide drawn in `mode`"""
    return int(width) | (int(mode) << 8)


_f32 = lambda x: C.c_float(x).value      # the defaults as the float32 fields hold them, so that get_spec() == SPEC_DEFAULTS
SPEC_DEFAULTS = dict(uniform_32bit=0, texel_gamma2=0, mis_single_lobe=0, eps_rule=0, eta_no_dielectric=1.0,
                     rr_start_bounce=3, rr_survival_cap=_f32(0.95), min_contribution=_f32(1.0e-2), min_throughput=_f32(1.0e-3), raygen_bilinear=0, env_orientation=0, display_gamma22=0)

METER_DEFAULTS = dict(key_stops=_f32(-2.4739311883324122), min_stops=-10.0, max_stops=10.0, white_permille=990, white_min=1.0, white_max=10.0, rect=(0, 0, 0, 0))      # key: log2(0.18)

OUTLINE_DEFAULTS = dict(kinds=OUTLINE_ALL, crease_cos=_f32(0.8660254037844387), depth_ratio=_f32(1.02), width=1, rgb=(0, 0, 0), alpha=255)      # cos 30 deg

DENOISE_DEFAULTS = dict(levels=4, normal_cos=_f32(0.9063077870366499), depth_ratio=_f32(1.05), until_samples=256)      # cos 25 deg

SHADE_GUIDE_DEFAULTS = dict(demodulate=1, lights=1, albedo_floor=0.015625, light_dilate=1)      # 1 / 64

VIEW_DEFAULTS = dict(width=0, height=0, src=(0, 0, 0, 0), filter=VIEW_AUTO, reserved=0)      # (a size must be given)

REPROJECT_DEFAULTS = dict(max_history=16.0, until_samples=64, normal_cos=_f32(0.9063077870366499), depth_ratio=_f32(1.05))      # cos 25 deg

ANNOT_DEFAULTS = dict(depth_bias=2.0 ** -9, hidden_alpha=64)

REPROJECT_MOTION_DEFAULTS = dict(max_history_moved=16.0, max_history_static=8.0)

assert C.sizeof(crh_outline_params) == 20 and C.sizeof(crh_denoise_params) == 16
assert C.sizeof(crh_shade_guide_params) == 16 and C.sizeof(crh_shade_guide_scene) == 56
assert C.sizeof(crh_reproject_params) == 16 and C.sizeof(crh_reproject_frame) == 64
assert C.sizeof(crh_reproject_motion_params) == 8
assert C.sizeof(crh_view_params) == 32
assert C.sizeof(crh_annot_segment) == 32 and C.sizeof(crh_annot_params) == 8
assert C.sizeof(crh_meter_params) == 40 and C.sizeof(crh_meter_result) == 1044
assert C.sizeof(crh_fit_result) == 84
assert C.sizeof(crh_region_stats) == 32
assert C.sizeof(crh_bsdf) == 128 and C.sizeof(crh_light) == 32 and C.sizeof(crh_spec) == 52

SCHEDULE_AUTO, SCHEDULE_WIDE, SCHEDULE_SMALL, SCHEDULE_STAGED = 0, 1, 2, 3      # crh_set_schedule

NODE_DWORDS = 16          # CRH_NODE_DWORDS of include/crh_bvh_format.h: 4-wide BVH node, 12 dwords used on a 64-B stride

# every symbol include/cadrays_hip.h declares (tests check the built library exports them all)
EXPORTS = [
    "crh_create", "crh_destroy", "crh_last_error", "crh_set_geometry", "crh_set_transforms", "crh_set_visibility", "crh_add_object", "crh_set_materials",
    "crh_set_lights", "crh_set_envmap", "crh_set_texture", "crh_set_camera", "crh_set_params", "crh_set_spec", "crh_get_spec", "crh_spec_order_exact", "crh_spec_anyhit_slot_order", "crh_build", "crh_reset",
    "crh_render", "crh_render_tiles", "crh_set_adaptive", "crh_set_show_tiles", "crh_set_lookahead", "crh_set_lookahead_auto", "crh_set_schedule", "crh_set_pipeline_depth", "crh_set_path_budget", "crh_get_tile_stats", "crh_sync", "crh_read_hdr", "crh_read_ldr", "crh_read_ldr_begin", "crh_read_ldr_end", "crh_read_hdr_begin", "crh_read_hdr_end",
    "crh_save_accum", "crh_load_accum", "crh_accum_device_ptr", "crh_reduce", "crh_enable_counters", "crh_get_stats", "crh_trace_nearest",
    "crh_trace_any", "crh_get_bvh", "crh_get_tlas", "crh_build_bvh_host", "crh_bench_trace", "crh_debug_math", "crh_debug_bsdf", "crh_enable_kernel_timing",
    "crh_get_kernel_timing", "crh_get_packet_stats", "crh_debug_reduce_fake_devices", "crh_get_path_budget", "crh_get_frame_tuning", "crh_get_tile_order", "crh_build_prebuilt", "crh_query_pipeline_capacity", "crh_env_table",
    "crh_camera_rays", "crh_pick", "crh_read_ids", "crh_set_selection", "crh_set_hover", "crh_get_selection_bounds",
    "crh_set_display", "crh_get_display", "crh_meter_defaults", "crh_meter_from_histogram", "crh_set_auto_exposure", "crh_measure_exposure",
    "crh_fit_view", "crh_fit_extents_host", "crh_fit_from_extents",
    "crh_query_region", "crh_region_stats_host", "crh_region_select",
    "crh_outline_defaults", "crh_set_outline", "crh_get_outline", "crh_read_outline", "crh_outline_table_host", "crh_outline_mask_host", "crh_outline_draw_host",
    "crh_denoise_defaults", "crh_set_denoise", "crh_get_denoise", "crh_read_denoised", "crh_denoise_host", "crh_bench_denoise",
    "crh_shade_guide_defaults", "crh_set_shade_guide", "crh_get_shade_guide", "crh_read_shade_guide", "crh_read_hit_uv", "crh_bench_shade_guide", "crh_guide_table_host",
    "crh_shade_guide_host", "crh_denoise_guided_host",
    "crh_reproject_defaults", "crh_set_reproject", "crh_get_reproject", "crh_read_reprojected", "crh_bench_reproject", "crh_reproject_frame_host", "crh_reproject_host",
    "crh_reproject_motion_defaults", "crh_set_reproject_motion", "crh_get_reproject_motion", "crh_get_reproject_launches", "crh_bench_reproject_motion", "crh_reproject_delta_host", "crh_reproject_motion_host",
    "crh_read_view", "crh_read_view_begin", "crh_read_view_end", "crh_view_host", "crh_view_fit", "crh_view_to_frame", "crh_bench_view",
    "crh_annot_defaults", "crh_set_annotations", "crh_get_annotations", "crh_read_annotation_ids", "crh_pick_annotation", "crh_read_annotation_records", "crh_bench_annotations",
    "crh_annot_project_host", "crh_annot_draw_host",
]
