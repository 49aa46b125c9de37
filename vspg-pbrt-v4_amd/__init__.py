"""vspg-pbrt-v4_amd -- Python plumbing over the C-ABI of the MI355X-native VSPG hot path.

The product is `csrc/libvspg_hip.so` (hand-written HIP kernels for gfx950 + the C-ABI declared
in include/vspg.h) and the C++ host adapter in `host/`.  This module is only a ctypes binding
used by tests/ and bench.py; it contains no algorithm and NO CPU fallback: if the shared
library is missing, `load()` raises.

The directory name carries a hyphen (it is the repo's package directory, not a Python
identifier); import it with `importlib` under the name `vspg_pbrt_v4_amd`
(see tests/conftest.py / bench.py: `load_package()`).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VSPG_LIB") or os.path.join(_HERE, "csrc", "libvspg_hip.so")  # VSPG_LIB: experiment builds (scripts/)

VSPG_MAX_QUADS = 16
VSPG_ISG_STATS = 8

MEDIUM_NONE, MEDIUM_HOMOGENEOUS, MEDIUM_GRID, MEDIUM_NANOVDB = 0, 1, 2, 3
MEDIUM_RGBGRID = 4      # VSPG_MEDIUM_RGBGRID: per-voxel RGB sigma_a / sigma_s / Le grids in the tail of VspgScene (set_rgb_grid_medium)
MEDIUM_POINT_OUT = 10   # VSPG_MEDIUM_POINT_OUT: floats per element of vspg_medium_point_batch
GUIDE_MIS, GUIDE_RIS = 0, 1
VSP_CONTRIBUTION, VSP_VARIANCE = 0, 1
VSP_RESAMPLING, VSP_NDS = 0, 1
LIGHTSAMPLER_UNIFORM, LIGHTSAMPLER_POWER, LIGHTSAMPLER_BVH = 0, 1, 2
TMAJ_PLAIN, TMAJ_OPTICAL_DEPTH, TMAJ_RESAMPLING = 0, 1, 2

VSPG_OK, VSPG_EINVAL, VSPG_ENODEVICE, VSPG_EHIP, VSPG_ESCOPE = 0, -1, -2, -3, -4
ARITH_EXACT, ARITH_FAST_WEIGHTS, ARITH_FAST = 0, 1, 2
GRID_DENSITY, GRID_TEMPERATURE = 0, 1  # VSPG_GRID_*: which grid vspg_renderer_update_grid replaces ...
MEM_HOST, MEM_DEVICE = 0, 1            # ... and VSPG_MEM_*: where its values live

f3 = C.c_float * 3


class VspgQuad(C.Structure):
    _fields_ = [("p00", f3), ("e1", f3), ("e2", f3), ("Kd", f3), ("Le", f3),
                ("two_sided", C.c_int32), ("reverse_orientation", C.c_int32),
                ("material", C.c_int32), ("medium_interface", C.c_int32)]


VSPG_MAX_SPHERES = 8
MATERIAL_DIFFUSE, MATERIAL_INTERFACE = 0, 1
IFACE_INSIDE, IFACE_OUTSIDE = 1, 2
TRI_INTERFACE, TRI_IFACE_SHIFT, TRI_FLIP_NORMAL = 1, 1, 8


class VspgSphere(C.Structure):
    _fields_ = [("render_from_object", C.c_float * 16), ("object_from_render", C.c_float * 16), ("radius", C.c_float),
                ("Kd", f3), ("reverse_orientation", C.c_int32), ("material", C.c_int32), ("medium_interface", C.c_int32)]


class VspgCamera(C.Structure):
    _fields_ = [("origin", f3), ("right", f3), ("up", f3), ("fwd", f3),
                ("sx", C.c_float), ("ox", C.c_float), ("sy", C.c_float), ("oy", C.c_float)]


CAMERA_PERSPECTIVE, CAMERA_ORTHOGRAPHIC, CAMERA_SPHERICAL_EQUALAREA, CAMERA_SPHERICAL_EQUIRECT = 0, 1, 2, 3   # VSPG_CAMERA_*


class VspgCameraModel(C.Structure):
    """The camera model of vspg_renderer_set_camera; zeroed = the pinhole perspective."""
    _fields_ = [("model", C.c_int32), ("lens_radius", C.c_float), ("focal_distance", C.c_float)]


class VspgMedium(C.Structure):
    _fields_ = [("type", C.c_int32), ("sigma_a", f3), ("sigma_s", f3), ("g", C.c_float),
                ("Le", f3), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32),
                ("bounds_min", f3), ("bounds_max", f3), ("density", C.POINTER(C.c_float)),
                ("index_min", C.c_int32 * 3), ("voxel_size", f3), ("grid_origin", f3),
                ("density_offset", C.c_float), ("majorant_scale", C.c_float),
                ("le_scale", C.POINTER(C.c_float)), ("le_nx", C.c_int32), ("le_ny", C.c_int32), ("le_nz", C.c_int32),
                ("has_transform", C.c_int32), ("render_from_medium", C.c_float * 16), ("medium_from_render", C.c_float * 16),
                ("temperature", C.POINTER(C.c_float)), ("nvdb_le_scale", C.c_float), ("temperature_offset", C.c_float),
                ("temperature_scale", C.c_float)]


VSPG_MAX_INFINITE_LIGHTS = 4
LIGHT_UNIFORM_INFINITE, LIGHT_DISTANT, LIGHT_IMAGE_INFINITE = 0, 1, 2
ENV_MAX_RES = 4096   # VSPG_ENV_MAX_RES
ENVLIGHT_OUT = 16    # VSPG_ENVLIGHT_OUT: floats per element of vspg_envlight_batch
PORTALLIGHT_OUT = 32  # VSPG_PORTALLIGHT_OUT: floats per element of vspg_portallight_batch


class VspgInfiniteLight(C.Structure):
    _fields_ = [("type", C.c_int32), ("L", f3), ("w_light", f3)]


VSPG_MAX_POINT_LIGHTS = 8
LIGHT_POINT, LIGHT_SPOT = 3, 4
LIGHT_PROJECTION, LIGHT_GONIOMETRIC = 5, 6   # image-shaped point lights, in the same VspgPointLight slots
LIGHT_IMAGE_MAX_RES = 4096                   # VSPG_LIGHT_IMAGE_MAX_RES
LIGHT_SAMPLE_OUT = 16  # VSPG_LIGHT_SAMPLE_OUT: floats per element of vspg_light_sample_batch
LIGHT_PDF_OUT = 8      # VSPG_LIGHT_PDF_OUT: floats per element of vspg_light_pdf_batch


class VspgPointLight(C.Structure):
    _fields_ = [("type", C.c_int32), ("I", f3), ("render_from_light", C.c_float * 16), ("light_from_render", C.c_float * 16),
                ("cone_angle_deg", C.c_float), ("cone_delta_deg", C.c_float)]


VSPG_MAX_TEXTURES = 8
TEXTURE_MAX_RES = 4096  # VSPG_TEXTURE_MAX_RES
TEXWRAP_REPEAT, TEXWRAP_CLAMP, TEXWRAP_BLACK = 0, 1, 2
TEXFILTER_POINT, TEXFILTER_BILINEAR = 0, 1
TEXTURE_EVAL_OUT = 8    # VSPG_TEXTURE_EVAL_OUT: floats per element of vspg_texture_eval_batch


class VspgTexture(C.Structure):
    _fields_ = [("pixels", C.POINTER(C.c_float)), ("xres", C.c_int32), ("yres", C.c_int32), ("channels", C.c_int32),
                ("wrap", C.c_int32), ("filter", C.c_int32), ("invert", C.c_int32), ("scale", C.c_float),
                ("su", C.c_float), ("sv", C.c_float), ("du", C.c_float), ("dv", C.c_float)]


class VspgScene(C.Structure):
    _fields_ = [("n_quads", C.c_int32), ("quads", VspgQuad * VSPG_MAX_QUADS),
                ("camera", VspgCamera), ("medium", VspgMedium),
                ("n_triangles", C.c_int32), ("tri_p", C.POINTER(C.c_float)), ("tri_kd", C.POINTER(C.c_float)),
                ("n_infinite_lights", C.c_int32), ("infinite_lights", VspgInfiniteLight * VSPG_MAX_INFINITE_LIGHTS),
                ("tri_flags", C.POINTER(C.c_int32)), ("n_spheres", C.c_int32), ("spheres", VspgSphere * VSPG_MAX_SPHERES),
                ("camera_outside_medium", C.c_int32),
                ("n_point_lights", C.c_int32), ("point_lights", VspgPointLight * VSPG_MAX_POINT_LIGHTS),
                ("sphere_Le", f3 * VSPG_MAX_SPHERES), ("sphere_two_sided", C.c_int32 * VSPG_MAX_SPHERES),
                ("rgb_sigma_a", C.POINTER(C.c_float)), ("rgb_sigma_s", C.POINTER(C.c_float)), ("rgb_Le", C.POINTER(C.c_float)),
                ("rgb_sigma_scale", C.c_float), ("rgb_le_scale", C.c_float)]


class VspgSceneTextures(C.Structure):
    """The record beside VspgScene that vspg_renderer_create_textured takes (scene_textures(scene) keeps one with a scene)."""
    _fields_ = [("n_textures", C.c_int32), ("textures", VspgTexture * VSPG_MAX_TEXTURES), ("quad_texture", C.c_int32 * VSPG_MAX_QUADS),
                ("tri_texture", C.POINTER(C.c_int32)), ("tri_uv", C.POINTER(C.c_float))]


class VspgIntegratorParams(C.Structure):
    _fields_ = [("maxdepth", C.c_int32), ("minrrdepth", C.c_int32), ("usenee", C.c_int32),
                ("surfaceguiding", C.c_int32), ("volumeguiding", C.c_int32),
                ("surfaceguidingtype", C.c_int32), ("volumeguidingtype", C.c_int32),
                ("vspguiding", C.c_int32), ("vspprimaryguiding", C.c_int32),
                ("vspsecondaryguiding", C.c_int32), ("vspmisratio", C.c_float),
                ("vspcriterion", C.c_int32), ("vspsamplingmethod", C.c_int32),
                ("collisionProbabilityBias", C.c_int32), ("rrguiding", C.c_int32),
                ("lightsampler", C.c_int32), ("regularize", C.c_int32),
                ("guide_num_training_waves", C.c_int32), ("storeTrBuffer", C.c_int32),
                ("surfacerrguiding", C.c_int32), ("volumerrguiding", C.c_int32)]


class VspgRenderConfig(C.Structure):
    _fields_ = [("xres", C.c_int32), ("yres", C.c_int32), ("spp", C.c_int32), ("seed", C.c_int32),
                ("shard_index", C.c_int32), ("shard_count", C.c_int32), ("device", C.c_int32)]


class VspgCounters(C.Structure):
    _fields_ = [("paths", C.c_uint64), ("segments", C.c_uint64), ("volume_scatters", C.c_uint64),
                ("surface_hits", C.c_uint64), ("density_queries", C.c_uint64),
                ("shadow_rays", C.c_uint64), ("shadow_density_queries", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class VspgFilmError(C.Structure):
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32), ("tag", C.c_int32),
                ("tick_khz", C.c_uint32), ("n_pixels", C.c_uint64), ("device_ticks", C.c_uint64),
                ("sum_se", C.c_double * 3), ("sum_rse", C.c_double * 3)]


FILM_ERROR_LOG_RECORDS = 4096


class FilmError:
    """One record of the film-error log (include/vspg.h, VspgFilmError): the six sums in double over a pixel window.  mse() /
    mrse() perform the reference's last step: per channel Float(sum / (Float(width) * Float(height))) (src/pbrt/util/image.cpp:603-606,
    :635-638), then ImageChannelValues::Average() in Float (image.h:205-210).  A record combined from several windows
    (sharding.combine_film_errors) is no rectangle: its divisor is Float(n_pixels)."""

    def __init__(self, x0, y0, x1, y1, tag, tick_khz, n_pixels, device_ticks, sum_se, sum_rse):
        self.x0, self.y0, self.x1, self.y1, self.tag = int(x0), int(y0), int(x1), int(y1), int(tag)
        self.tick_khz, self.n_pixels, self.device_ticks = int(tick_khz), int(n_pixels), int(device_ticks)
        self.sum_se, self.sum_rse = [float(v) for v in sum_se], [float(v) for v in sum_rse]

    @classmethod
    def from_c(cls, rec):
        return cls(rec.x0, rec.y0, rec.x1, rec.y1, rec.tag, rec.tick_khz, rec.n_pixels, rec.device_ticks, list(rec.sum_se),
                   list(rec.sum_rse))

    def window(self):
        return self.x0, self.y0, self.x1, self.y1

    def channel_means(self, sums):
        import numpy as np
        if self.n_pixels == (self.x1 - self.x0) * (self.y1 - self.y0):
            div = np.float32(self.x1 - self.x0) * np.float32(self.y1 - self.y0)
        else:
            div = np.float32(self.n_pixels)
        with np.errstate(all="ignore"):
            return [np.float32(np.float64(s) / np.float64(div)) for s in sums]   # double / Float, stored as Float

    def _average(self, sums):
        import numpy as np
        acc = np.float32(0)
        with np.errstate(all="ignore"):
            for v in self.channel_means(sums):
                acc = np.float32(acc + v)
            return float(np.float32(acc / np.float32(3)))

    def mse(self):
        return self._average(self.sum_se)

    def mrse(self):
        return self._average(self.sum_rse)

    def __repr__(self):
        return "FilmError(window=%r, tag=%d, n_pixels=%d, sum_se=%r, sum_rse=%r, device_ticks=%d)" % (
            self.window(), self.tag, self.n_pixels, self.sum_se, self.sum_rse, self.device_ticks)


class VspgTrainSample(C.Structure):
    _fields_ = [("p", C.c_float * 3), ("dir", C.c_float * 3), ("weight", C.c_float), ("pdf", C.c_float),
                ("distance", C.c_float), ("flags", C.c_uint32)]


class VspgTrainStats(C.Structure):
    _fields_ = [("training", C.c_int32), ("iteration", C.c_int32), ("n_samples", C.c_uint64), ("n_zero", C.c_uint64),
                ("n_nodes", C.c_int32 * 2), ("n_regions", C.c_int32 * 2), ("n_dropped", C.c_uint64)]

    def as_dict(self):
        return {"training": int(self.training), "iteration": int(self.iteration), "n_samples": int(self.n_samples),
                "n_zero": int(self.n_zero), "n_nodes": list(self.n_nodes), "n_regions": list(self.n_regions),
                "n_dropped": int(self.n_dropped)}


TRAIN_SAMPLE_DTYPE = [("p", "<f4", 3), ("dir", "<f4", 3), ("weight", "<f4"), ("pdf", "<f4"), ("distance", "<f4"),
                      ("flags", "<u4")]

VSPG_FIELD_LOBES = 8
_fl = C.c_float * VSPG_FIELD_LOBES


class VspgKdNode(C.Structure):
    _fields_ = [("split", C.c_float), ("packed", C.c_uint32)]


class VspgFieldRegion(C.Structure):
    _fields_ = [("pivot", f3), ("n_lobes", C.c_int32), ("weight", _fl), ("kappa", _fl), ("mu", _fl * 3),
                ("distance", _fl), ("vsp", _fl)]


class VspgField(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("n_regions", C.c_int32), ("nodes", C.POINTER(VspgKdNode)),
                ("regions", C.POINTER(VspgFieldRegion))]


class VspgTmajQuery(C.Structure):
    _fields_ = [("o", f3), ("d", f3), ("tMax", C.c_float), ("u", C.c_float),
                ("rng_a", C.c_float), ("rng_b", C.c_float), ("vsp", C.c_float),
                ("channel", C.c_int32), ("stop_after", C.c_int32)]


class VspgRayQuery(C.Structure):
    _fields_ = [("o", f3), ("d", f3), ("tMax", C.c_float), ("mode", C.c_int32), ("w", f3), ("tMax2", C.c_float)]


class VspgRayResult(C.Structure):
    _fields_ = [("hit", C.c_int32), ("prim", C.c_int32), ("t", C.c_float), ("p", f3), ("n", f3), ("o2", f3), ("d2", f3),
                ("hit2", C.c_int32), ("any2", C.c_int32), ("t2", C.c_float)]


RAY_QUERY_DTYPE = [("o", "<f4", 3), ("d", "<f4", 3), ("tMax", "<f4"), ("mode", "<i4"), ("w", "<f4", 3), ("tMax2", "<f4")]
RAY_RESULT_DTYPE = [("hit", "<i4"), ("prim", "<i4"), ("t", "<f4"), ("p", "<f4", 3), ("n", "<f4", 3), ("o2", "<f4", 3), ("d2", "<f4", 3),
                    ("hit2", "<i4"), ("any2", "<i4"), ("t2", "<f4")]


class VspgTmajResult(C.Structure):
    _fields_ = [("T_maj", f3), ("r_u_factor", f3), ("last_t", C.c_float), ("last_p", f3),
                ("n_callbacks", C.c_int32), ("sum_sigt_over_maj", C.c_float),
                ("vrc", C.c_float), ("majorant_scale", C.c_float)]


class VspgBrickInfo(C.Structure):
    _fields_ = [("bnx", C.c_int32), ("bny", C.c_int32), ("bnz", C.c_int32), ("indexed", C.c_int32),
                ("n_stored", C.c_uint64), ("index_bytes", C.c_uint64), ("octet_bytes", C.c_uint64)]


RESOLVE_F32, RESOLVE_F16 = 0, 1           # VSPG_RESOLVE_*: the format ...
RESOLVE_RGB, RESOLVE_SCANLINE_BGR = 0, 1  # ... and the layout of vspg_film_resolve

# every symbol include/vspg.h declares: (name, restype, argtypes)
_P = C.POINTER
_vp = C.c_void_p
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p)   # VspgExchangeFn
SYMBOLS = [
    ("vspg_abi_version", C.c_int, []),
    ("vspg_last_error", C.c_char_p, []),
    ("vspg_integrator_params_default", None, [_P(VspgIntegratorParams)]),
    ("vspg_camera_look_at", C.c_int, [_P(VspgCamera), f3, f3, f3, C.c_float, C.c_int, C.c_int]),
    ("vspg_scene_fog_box", C.c_int, [_P(VspgScene), C.c_int, C.c_int]),
    ("vspg_transform_inverse", C.c_int, [C.c_float * 16, C.c_float * 16]),
    ("vspg_renderer_create", C.c_int, [_P(VspgScene), _P(VspgIntegratorParams), _P(VspgRenderConfig), _P(_vp)]),
    ("vspg_renderer_create_textured", C.c_int, [_P(VspgScene), _P(VspgSceneTextures), _P(VspgIntegratorParams), _P(VspgRenderConfig), _P(_vp)]),
    ("vspg_renderer_destroy", C.c_int, [_vp]),
    ("vspg_render_wave", C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    ("vspg_render_window", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
    ("vspg_post_process_wave", C.c_int, [_vp, _vp]),
    ("vspg_isg_update_due", C.c_int, [_vp, C.c_int]),
    ("vspg_post_process_step", C.c_int, [_vp, C.c_int, _vp, _vp]),
    ("vspg_renderer_set_exchange", C.c_int, [_vp, _vp, _vp]),
    ("vspg_renderer_kernel_name", C.c_char_p, [_vp]),
    ("vspg_ray_batch", C.c_int, [_vp, C.c_int, _P(VspgRayQuery), _P(VspgRayResult), _vp]),
    ("vspg_renderer_set_arithmetic", C.c_int, [_vp, C.c_int]),
    ("vspg_renderer_get_arithmetic", C.c_int, [_vp]),
    ("vspg_flush", C.c_int, [_vp, _vp]),
    ("vspg_film_device_ptr", C.c_int, [_vp, _P(_vp), _P(C.c_size_t)]),
    ("vspg_film_read", C.c_int, [_vp, _P(C.c_float), _vp]),
    ("vspg_film_clear", C.c_int, [_vp, _vp]),
    ("vspg_renderer_set_reference_image", C.c_int, [_vp, _P(C.c_float), _vp]),
    ("vspg_film_error_enqueue", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
    ("vspg_film_error_read", C.c_int, [_vp, _P(VspgFilmError), C.c_size_t, _P(C.c_size_t), _vp]),
    ("vspg_film_resolve", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_size_t, _P(C.c_uint64), _vp]),
    ("vspg_vsp_buffer_device_ptr", C.c_int, [_vp, _P(_vp), _P(C.c_size_t)]),
    ("vspg_vsp_buffer_read", C.c_int, [_vp, _P(C.c_float), _P(C.c_int), _vp]),
    ("vspg_vsp_buffer_load", C.c_int, [_vp, _P(C.c_float), _vp]),
    ("vspg_isg_stats_device_ptr", C.c_int, [_vp, _P(_vp), _P(C.c_size_t)]),
    ("vspg_get_counters", C.c_int, [_vp, _P(VspgCounters), _vp]),
    ("vspg_reset_counters", C.c_int, [_vp, _vp]),
    ("vspg_trace_paths", C.c_int, [_vp, C.c_int, _P(C.c_int32), _P(C.c_int32), _P(C.c_float), _P(C.c_int32), _vp]),
    ("vspg_sample_tmaj_batch", C.c_int, [_vp, C.c_int, C.c_int, _P(VspgTmajQuery), _P(VspgTmajResult), _vp]),
    ("vspg_brick_info", C.c_int, [_vp, _P(VspgBrickInfo)]),
    ("vspg_brick_read", C.c_int, [_vp, _P(C.c_int32), _P(C.c_float), _vp]),
    ("vspg_renderer_update_grid", C.c_int, [_vp, C.c_int, _vp, C.c_size_t, C.c_int, _vp]),
    ("vspg_renderer_update_rgb_grids", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, C.c_int, _vp]),
    ("vspg_rgb_octets_read", C.c_int, [_vp, C.c_int, _P(C.c_float), C.c_size_t, _vp]),
    ("vspg_majorant_read", C.c_int, [_vp, _P(C.c_float), C.c_size_t, _P(C.c_int32), _vp]),
    ("vspg_medium_point_batch", C.c_int, [_vp, C.c_int, _P(C.c_float), _P(C.c_float), _vp]),
    ("vspg_primitives_batch", C.c_int, [_vp, C.c_int, _P(C.c_float), _P(C.c_float), _P(C.c_uint64), _P(C.c_uint32), _P(C.c_float), _vp]),
    ("vspg_renderer_training_stats", C.c_int, [_vp, _P(VspgTrainStats), _vp]),
    ("vspg_train_samples_read", C.c_int, [_vp, _P(VspgTrainSample), C.c_size_t, _P(C.c_size_t), _vp]),
    ("vspg_renderer_get_guiding_field", C.c_int, [_vp, C.c_int, _P(VspgKdNode), _P(VspgFieldRegion), _P(C.c_int32),
                                                  _P(C.c_int32), _vp]),
    ("vspg_libm_batch", C.c_int, [_vp, C.c_int, _P(C.c_float), _P(C.c_float), _P(C.c_float), _P(C.c_float), _vp]),
    ("vspg_libm_log1m_batch", C.c_int, [_vp, C.c_int, _P(C.c_float), _P(C.c_float), _vp]),
    ("vspg_libm_powf_batch", C.c_int, [_vp, C.c_int, _P(C.c_float), _P(C.c_float), _P(C.c_float), _vp]),
    ("vspg_blackbody_batch", C.c_int, [_vp, C.c_int, _P(C.c_float), _P(C.c_float), _P(C.c_float), _vp]),
    ("vspg_renderer_set_environment_image", C.c_int, [_vp, C.c_int, _P(C.c_float), C.c_int, _P(C.c_float), _vp]),
    ("vspg_envlight_batch", C.c_int, [_vp, C.c_int, C.c_int, _P(C.c_float), _P(C.c_float), _P(C.c_float), _vp]),
    ("vspg_renderer_set_portal_environment_image", C.c_int, [_vp, C.c_int, _P(C.c_float), C.c_int, _P(C.c_float), _P(C.c_float), _vp]),
    ("vspg_portallight_batch", C.c_int, [_vp, C.c_int, C.c_int, _P(C.c_float), _P(C.c_float), _P(C.c_float), _P(C.c_float), _vp]),
    ("vspg_portallight_read", C.c_int, [_vp, C.c_int, _P(C.c_int), _P(C.c_float), _P(C.c_float), _P(C.c_float), _P(C.c_float), _vp]),
    ("vspg_spot_light_look_at", C.c_int, [_P(VspgPointLight), f3, f3, _P(C.c_float)]),
    ("vspg_point_light_at", C.c_int, [_P(VspgPointLight), f3, _P(C.c_float)]),
    ("vspg_projection_light_at", C.c_int, [_P(VspgPointLight), _P(C.c_float)]),
    ("vspg_goniometric_light_at", C.c_int, [_P(VspgPointLight), _P(C.c_float)]),
    ("vspg_renderer_set_light_image", C.c_int, [_vp, C.c_int, _P(C.c_float), C.c_int, C.c_int, C.c_int, _vp]),
    ("vspg_light_sample_batch", C.c_int, [_vp, C.c_int, _P(C.c_float), _P(C.c_float), _P(C.c_float), _P(C.c_float), _vp]),
    ("vspg_light_pdf_batch", C.c_int, [_vp, C.c_int, C.c_int, _P(C.c_float), _P(C.c_float), _P(C.c_float), _P(C.c_float), _P(C.c_float), _vp]),
    ("vspg_renderer_set_texture_image", C.c_int, [_vp, C.c_int, _P(C.c_float), C.c_int, C.c_int, C.c_int, _vp]),
    ("vspg_texture_eval_batch", C.c_int, [_vp, C.c_int, _P(C.c_int32), _P(C.c_float), _P(C.c_float), _vp]),
    ("vspg_renderer_set_camera", C.c_int, [_vp, _P(VspgCamera), _P(VspgCameraModel), _vp]),
    ("vspg_camera_look_at_window", C.c_int, [_P(VspgCamera), C.c_int, f3, f3, f3, C.c_float, _P(C.c_float), C.c_float, C.c_int, C.c_int]),
    ("vspg_camera_ray_batch", C.c_int, [_vp, C.c_int, _P(C.c_int32), _P(C.c_int32), _P(C.c_float), _P(C.c_float), _P(C.c_float), _vp]),
    ("vspg_renderer_get_tr_buffer", C.c_int, [_vp, _P(C.c_float), _P(C.c_int32), _vp]),
    ("vspg_renderer_set_tr_buffer", C.c_int, [_vp, _P(C.c_float), _vp]),
    ("vspg_renderer_set_guiding_field", C.c_int, [_vp, _P(VspgField), _P(VspgField), _vp]),
    ("vspg_guiding_query_batch", C.c_int, [_vp, C.c_int, C.c_float, C.c_int, _P(C.c_float), _P(C.c_float), _P(C.c_float),
                                          _P(C.c_float), _P(C.c_int32), _P(C.c_float), _P(C.c_float), _P(C.c_float),
                                          _P(C.c_float), _P(C.c_float), _vp]),
]

_lib = None


class VspgError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("vspg error %d: %s" % (code, msg))
        self.code = code


def load():
    """Load csrc/libvspg_hip.so (built by __graft_entry__.build()).  Raises if it is missing:
    there is no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`"
                           % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _check(lib, rc):
    if rc != 0:
        raise VspgError(rc, (lib.vspg_last_error() or b"").decode())


def default_params():
    lib = load()
    p = VspgIntegratorParams()
    lib.vspg_integrator_params_default(C.byref(p))
    return p


def fog_box_scene(xres, yres):
    lib = load()
    s = VspgScene()
    _check(lib, lib.vspg_scene_fog_box(C.byref(s), xres, yres))
    return s


def camera_look_at_window(model, eye, look, up, fov, xres, yres, screen_window=None, frame_aspect=0.0):
    """A VspgCamera for camera model `model` (CAMERA_*): LookAt and the model's screen window (vspg_camera_look_at_window).
    screen_window: (xmin, xmax, ymin, ymax) or None = the default window of frame_aspect (0 = xres / yres)."""
    lib = load()
    cam = VspgCamera()
    sw = None if screen_window is None else (C.c_float * 4)(*[float(v) for v in screen_window])
    _check(lib, lib.vspg_camera_look_at_window(C.byref(cam), int(model), f3(*eye), f3(*look), f3(*up), float(fov), sw, float(frame_aspect),
                                               int(xres), int(yres)))
    return cam


def procedural_cloud_density(n, seed=5, shape="noise"):
    """Seeded value noise, density in [0, ~1.3], ~25-30 % empty voxels, x fastest (the layout
    cmd/nanovdb2pbrt.cpp dumps for GridMedium): the heterogeneous stand-in of SURVEY.md 8d until a
    Disney-cloud asset is supplied.  shape="blob": the same noise inside a soft-edged ball of radius 0.36 n around the
    grid's centre and nothing outside it (~80 % empty voxels, empty majorant cells all around: what a real cloud in
    its bounding box looks like to the majorant grid)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    coarse = rng.random((n // 4 + 2,) * 3).astype(np.float32)
    idx = (np.arange(n, dtype=np.float32) + 0.5) / 4.0
    i0 = np.floor(idx).astype(int)
    f = (idx - i0).astype(np.float32)

    def interp(a, axis):
        shape = [1, 1, 1]
        shape[axis] = n
        w = f.reshape(shape)
        return np.take(a, i0, axis=axis) * (1 - w) + np.take(a, i0 + 1, axis=axis) * w

    v = interp(interp(interp(coarse, 0), 1), 2)
    v = np.clip(v * 2.2 - 0.75, 0.0, None)
    if shape == "blob":
        c = (np.arange(n, dtype=np.float32) + 0.5) / n - 0.5
        r = np.sqrt(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2)
        v = (v + 0.35) * np.clip((0.36 - r) / 0.06, 0.0, 1.0).astype(np.float32)
    return np.ascontiguousarray(v.transpose(2, 1, 0).reshape(-1).astype(np.float32))


def cloud_box_scene(xres, yres, n=256, sigma_t=8.0, albedo=0.99, g=0.877, seed=5, shape="noise"):
    """Fog-box geometry and light with the homogeneous fog replaced by a procedural n^3 GridMedium
    (sigma_t scale 8, albedo 0.99, g 0.877 -- SURVEY.md 8d's cloud-like choice)."""
    s = fog_box_scene(xres, yres)
    dens = procedural_cloud_density(n, seed, shape)
    m = s.medium
    m.type = MEDIUM_GRID
    m.sigma_a[:] = (sigma_t * (1 - albedo),) * 3
    m.sigma_s[:] = (sigma_t * albedo,) * 3
    m.g = g
    m.nx = m.ny = m.nz = n
    m.bounds_min[:] = (-0.9, -0.9, -0.6)
    m.bounds_max[:] = (0.9, 0.8, 0.9)
    m.density = dens.ctypes.data_as(C.POINTER(C.c_float))
    s._density_keepalive = dens
    return s


def nanovdb_box_scene(xres, yres, n=256, sigma_t=8.0, albedo=0.99, g=0.877, seed=5, density_offset=0.0, majorant_scale=1.0, shape="noise"):
    """Same cloud, handed over as a NanoVDBMedium (dense copy): index bbox [0, n-1]^3, cubic voxels, the world
    bounding box covers the voxel extents (what cmd/nanovdb2pbrt.cpp reads from the grid); 64^3 majorants."""
    s = cloud_box_scene(xres, yres, n, sigma_t, albedo, g, seed, shape)
    m = s.medium
    m.type = MEDIUM_NANOVDB
    ext = [m.bounds_max[k] - m.bounds_min[k] for k in range(3)]
    for k in range(3):
        m.index_min[k] = 0
        m.voxel_size[k] = ext[k] / n
        m.grid_origin[k] = m.bounds_min[k]
    m.density_offset = density_offset
    m.majorant_scale = majorant_scale
    return s


def add_quad(scene, p00, e1, e2, kd=(0.5, 0.5, 0.5), le=(0, 0, 0), material=0, iface=0, reverse=0, two_sided=0):
    """One more rectangle p00 + u e1 + v e2 (normal = normalize(e1 x e2), negated by `reverse`); material / iface: MATERIAL_*, IFACE_*."""
    k = scene.n_quads
    assert k < VSPG_MAX_QUADS
    q = scene.quads[k]
    q.p00[:] = p00
    q.e1[:] = e1
    q.e2[:] = e2
    q.Kd[:] = kd
    q.Le[:] = le
    q.two_sided, q.reverse_orientation, q.material, q.medium_interface = two_sided, reverse, material, iface
    scene.n_quads = k + 1
    return scene


def add_sphere(scene, center, radius, material=0, iface=0, kd=(0.5, 0.5, 0.5), scale=(1, 1, 1), reverse=0):
    """Shape "sphere" under Translate(center) * Scale(scale)."""
    import numpy as np
    k = scene.n_spheres
    assert k < VSPG_MAX_SPHERES
    sp = scene.spheres[k]
    m = np.eye(4, dtype=np.float32)
    m[0, 0], m[1, 1], m[2, 2] = scale
    m[0, 3], m[1, 3], m[2, 3] = center
    sp.render_from_object[:] = [float(x) for x in m.reshape(16)]
    # the inverse as the header and the scene-file reader form it (vspg_transform_inverse: pbrt's float Inverse(), transform.cpp):
    # the same scaled sphere gets the same matrix bits -- and so the same interval-arithmetic hits -- whichever way it came in
    inv = (C.c_float * 16)()
    lib = load()
    _check(lib, lib.vspg_transform_inverse(sp.render_from_object, inv))
    sp.object_from_render[:] = list(inv)
    sp.radius = radius
    sp.Kd[:] = kd
    sp.reverse_orientation, sp.material, sp.medium_interface = reverse, material, iface
    scene.n_spheres = k + 1
    return scene


def cloud_scene(xres, yres, n=256, sigma_t=8.0, albedo=0.99, g=0.877, seed=5, shape="noise", nvdb=False):
    """The shape of the reference's cloud scenes (BASELINE configs 3-5): the camera in VACUUM, the procedural n^3 cloud inside an
    interface-material bounding sphere (MediumInterface "cloud" "" + Material "interface"), a diffuse ground under it, a
    distant light and a uniform sky -- no closed box, no emissive geometry."""
    lib = load()
    s = VspgScene()
    _check(lib, lib.vspg_camera_look_at(C.byref(s.camera), f3(0.0, 0.6, -4.2), f3(0.0, 0.15, 0.0), f3(0, 1, 0), 38.0, xres, yres))
    dens = procedural_cloud_density(n, seed, shape)
    m = s.medium
    m.type = MEDIUM_NANOVDB if nvdb else MEDIUM_GRID
    m.sigma_a[:] = (sigma_t * (1 - albedo),) * 3
    m.sigma_s[:] = (sigma_t * albedo,) * 3
    m.g = g
    m.nx = m.ny = m.nz = n
    m.bounds_min[:] = (-0.8, -0.5, -0.8)
    m.bounds_max[:] = (0.8, 0.9, 0.8)
    m.density = dens.ctypes.data_as(C.POINTER(C.c_float))
    s._density_keepalive = dens
    if nvdb:
        for k in range(3):
            m.index_min[k] = 0
            m.voxel_size[k] = (m.bounds_max[k] - m.bounds_min[k]) / n
            m.grid_origin[k] = m.bounds_min[k]
        m.density_offset = 0.0
        m.majorant_scale = 1.0
    s.camera_outside_medium = 1
    add_sphere(s, (0.0, 0.2, 0.0), 1.34, material=MATERIAL_INTERFACE, iface=IFACE_INSIDE)
    add_quad(s, (-6, -1.2, -6), (0, 0, 12), (12, 0, 0), kd=(0.4, 0.35, 0.3))   # ground, n = +y
    add_infinite_light(s, LIGHT_DISTANT, (6.0, 5.5, 5.0), (0.4, 0.8, -0.3))
    add_infinite_light(s, LIGHT_UNIFORM_INFINITE, (0.25, 0.35, 0.5))
    return s


def set_rgb_grid_medium(scene, sigma_a=None, sigma_s=None, Le=None, p0=(0, 0, 0), p1=(1, 1, 1), g=0.0, scale=1.0, Lescale=1.0):
    """Makes the scene's medium an RGBGridMedium ("rgbgrid"; parameter names and defaults of RGBGridMedium::Create,
    src/pbrt/media.cpp:411-484).  sigma_a / sigma_s / Le: arrays of shape (nz, ny, nx, 3) -- x fastest, R G B per voxel -- or None
    (absent: an absent sigma grid counts as the constant 1); all of one shape.  The arrays are kept alive on the scene."""
    import numpy as np
    grids = {}
    shape = None
    for name, a in (("sigma_a", sigma_a), ("sigma_s", sigma_s), ("Le", Le)):
        if a is None:
            continue
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim != 4 or a.shape[3] != 3:
            raise ValueError("%s must have shape (nz, ny, nx, 3)" % name)
        if shape is not None and a.shape != shape:
            raise ValueError("Different number of samples provided for the grids of an RGB grid medium")
        shape = a.shape
        grids[name] = a
    m = scene.medium
    m.type = MEDIUM_RGBGRID
    m.g = g
    if shape is not None:
        m.nz, m.ny, m.nx = shape[:3]
    m.bounds_min[:] = p0
    m.bounds_max[:] = p1
    null = C.POINTER(C.c_float)()
    scene.rgb_sigma_a = grids["sigma_a"].ctypes.data_as(C.POINTER(C.c_float)) if "sigma_a" in grids else null
    scene.rgb_sigma_s = grids["sigma_s"].ctypes.data_as(C.POINTER(C.c_float)) if "sigma_s" in grids else null
    scene.rgb_Le = grids["Le"].ctypes.data_as(C.POINTER(C.c_float)) if "Le" in grids else null
    scene.rgb_sigma_scale = scale
    scene.rgb_le_scale = Lescale
    scene._rgb_keepalive = grids
    return scene


def set_medium_transform(scene, m):
    """renderFromMedium = the row-major 4x4 `m` (affine); the inverse is filled by vspg_transform_inverse."""
    import numpy as np
    lib = load()
    a = (C.c_float * 16)(*[float(x) for x in np.asarray(m, dtype=np.float32).reshape(16)])
    inv = (C.c_float * 16)()
    _check(lib, lib.vspg_transform_inverse(a, inv))
    scene.medium.has_transform = 1
    scene.medium.render_from_medium[:] = list(a)
    scene.medium.medium_from_render[:] = list(inv)
    return scene


def add_infinite_light(scene, kind, L, w_light=(0.0, 1.0, 0.0)):
    """kind: LIGHT_UNIFORM_INFINITE (sky, radiance L), LIGHT_DISTANT (sun, radiance L from direction w_light, normalised here) or
    LIGHT_IMAGE_INFINITE (environment map: L multiplies the texels; the image is given to the renderer, Renderer.set_environment_image)."""
    import numpy as np
    k = scene.n_infinite_lights
    assert k < VSPG_MAX_INFINITE_LIGHTS
    w = np.asarray(w_light, dtype=np.float64)
    w = (w / np.linalg.norm(w)).astype(np.float32)
    il = scene.infinite_lights[k]
    il.type = kind
    il.L[:] = [float(x) for x in L]
    il.w_light[:] = [float(x) for x in w]
    scene.n_infinite_lights = k + 1
    return scene


def _add_point_light(scene, kind, I, scale, fill_transform):
    """Appends a VspgPointLight of `kind` with I * scale (float32, as the host multiplies them out) and lets `fill_transform(light)` fill
    both matrices; returns the light's index among the scene's point lights."""
    import numpy as np
    if scene.n_point_lights >= VSPG_MAX_POINT_LIGHTS:
        raise ValueError("too many point lights (VSPG_MAX_POINT_LIGHTS = %d)" % VSPG_MAX_POINT_LIGHTS)
    l = scene.point_lights[scene.n_point_lights]
    l.type = kind
    for k in range(3):
        l.I[k] = np.float32(I[k]) * np.float32(scale)
    _check(load(), fill_transform(l))
    scene.n_point_lights += 1
    return scene.n_point_lights - 1


def _ctm_pointer(ctm):
    import numpy as np
    if ctm is None:
        return None, None
    a = np.ascontiguousarray(np.asarray(ctm, dtype=np.float32).reshape(16))
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def add_point_light(scene, I, from_, scale=1, power=None, ctm=None):
    """LightSource "point" (PointLight::Create, lights.cpp:224-248): intensity I (RGB) times `scale`, at `from_` under the current
    transformation matrix `ctm` (4 x 4 row-major, None = identity).  power > 0 rescales as Create does: scale *= power / (4 Pi)."""
    import numpy as np
    lib = load()
    sc = np.float32(scale)
    if power is not None and power > 0:
        sc = sc * (np.float32(power) / (np.float32(4) * np.float32(np.pi)))
    keep, cp = _ctm_pointer(ctm)
    return _add_point_light(scene, LIGHT_POINT, I, sc, lambda l: lib.vspg_point_light_at(C.byref(l), f3(*[float(v) for v in from_]), cp))


def add_spot_light(scene, I, from_, to, coneangle=30, conedelta=5, scale=1, power=None, ctm=None):
    """LightSource "spot" (SpotLight::Create, lights.cpp:1520-1555): intensity I (RGB) times `scale`, at `from_` shining towards `to`
    under `ctm`; full intensity inside coneangle - conedelta degrees of the axis, a smooth falloff to zero at coneangle.  power > 0
    rescales as Create does: scale *= power / (2 Pi ((1 - cosStart) + (cosStart - cosEnd) / 2))."""
    import numpy as np
    lib = load()
    one, two = np.float32(1), np.float32(2)
    sc = np.float32(scale)
    if power is not None and power > 0:
        rad = np.float32(np.pi) / np.float32(180)
        ce = np.cos(rad * np.float32(coneangle))
        cs = np.cos(rad * (np.float32(coneangle) - np.float32(conedelta)))
        sc = sc * (np.float32(power) / (two * np.float32(np.pi) * ((one - cs) + (cs - ce) / two)))

    def fill(l):
        l.cone_angle_deg, l.cone_delta_deg = coneangle, conedelta
        return lib.vspg_spot_light_look_at(C.byref(l), f3(*[float(v) for v in from_]), f3(*[float(v) for v in to]), cp)
    keep, cp = _ctm_pointer(ctm)
    return _add_point_light(scene, LIGHT_SPOT, I, sc, fill)


def add_projection_light(scene, I, fov=90, ctm=None):
    """LightSource "projection" (ProjectionLight::Create, lights.cpp:490-560): a slide projector at the origin of `ctm` looking along its
    +z, I = the reference's `scale` as an RGB multiplier of the slide's texels, `fov` degrees across the slide's shorter axis.  The
    slide is given to the renderer (Renderer.set_light_image; a 1 x 1 slide of ones until then).  No "power": its normalisation needs
    the colour space's LuminanceVector."""
    lib = load()
    keep, cp = _ctm_pointer(ctm)
    def fill(l):
        l.cone_angle_deg = fov      # a projection slot's cone_angle_deg is its field of view (include/vspg.h)
        return lib.vspg_projection_light_at(C.byref(l), cp)
    return _add_point_light(scene, LIGHT_PROJECTION, I, 1, fill)


def add_goniometric_light(scene, I, scale=1, power=None, ctm=None, image=None):
    """LightSource "goniometric" (GoniometricLight::Create, lights.cpp:652-734): a bulb at the origin of `ctm` whose intensity is I (RGB)
    times `scale` times a texel of a square equal-area map, given to the renderer (Renderer.set_light_image; a 1 x 1 map of ones -- a
    point light -- until then).  power > 0 rescales as Create does: scale *= power / (4 Pi sumY / (width * height)), with the sum over
    `image` (the [res, res] map the renderer will be given) or over the 1 x 1 map of ones."""
    import numpy as np
    lib = load()
    sc = np.float32(scale)
    if power is not None and power > 0:
        sum_y, n = np.float32(1), 1
        if image is not None:
            img = np.asarray(image, dtype=np.float32).reshape(-1)
            sum_y, n = np.float32(0), img.size
            for v in img:
                sum_y = sum_y + v
        k_e = np.float32(4) * np.float32(np.pi) * sum_y / np.float32(n)
        sc = sc * (np.float32(power) / k_e)
    keep, cp = _ctm_pointer(ctm)
    return _add_point_light(scene, LIGHT_GONIOMETRIC, I, sc, lambda l: lib.vspg_goniometric_light_at(C.byref(l), cp))


def add_sphere_light(scene, sphere_index, L, scale=1, two_sided=False, power=None):
    """AreaLightSource "diffuse" on sphere `sphere_index` of the scene (DiffuseAreaLight::Create, lights.cpp:906-993): emitted radiance L
    (RGB) times `scale`.  power > 0 rescales as Create does (lights.cpp:969-990): scale *= power / k_e with k_e = (two_sided ? 2 : 1) *
    Area() * Pi, Area() = phiMax * radius * (zMax - zMin) in object space.  No photometric factor, as for the other lights here.
    Returns the light's index among the scene's emissive spheres (so far)."""
    import numpy as np
    if not 0 <= sphere_index < scene.n_spheres:
        raise ValueError("sphere_index %d outside the scene's %d spheres" % (sphere_index, scene.n_spheres))
    f = np.float32
    sc = f(scale)
    if power is not None and power > 0:
        r = f(scene.spheres[sphere_index].radius)
        phi_max = (f(np.pi) / f(180)) * f(360)
        area = (phi_max * r) * (r - (-r))
        k_e = f(1) * (f(2 if two_sided else 1) * area * f(np.pi))
        sc = sc * (f(power) / k_e)
    for k in range(3):
        scene.sphere_Le[sphere_index][k] = f(L[k]) * sc
    scene.sphere_two_sided[sphere_index] = 1 if two_sided else 0
    return sum(1 for i in range(sphere_index) if any(scene.sphere_Le[i][k] != 0 for k in range(3)))


def set_triangles(scene, tri_p, tri_kd=None):
    """Attach a triangle soup (n x 3 x 3 vertex array, optional n x 3 diffuse reflectances) to the scene."""
    import numpy as np
    tp = np.ascontiguousarray(tri_p, dtype=np.float32).reshape(-1, 9)
    scene.n_triangles = tp.shape[0]
    scene.tri_p = tp.ctypes.data_as(C.POINTER(C.c_float))
    scene._tri_keepalive = [tp]
    if tri_kd is not None:
        tk = np.ascontiguousarray(tri_kd, dtype=np.float32).reshape(-1, 3)
        assert tk.shape[0] == tp.shape[0]
        scene.tri_kd = tk.ctypes.data_as(C.POINTER(C.c_float))
        scene._tri_keepalive.append(tk)
    return scene


def texture_image_source(image):
    """What a texture's image is handed over as: a C-contiguous float32 NumPy array [yres, xres] or [yres, xres, 1] (grey) or
    [yres, xres, 3] (R, G, B), top row first.  A torch tensor (on any device) is copied to such an array.  Anything else raises
    ValueError -- here, before the library is called; the library judges the resolution and the texel values.
    Returns (array, xres, yres, channels)."""
    import numpy as np
    if type(image).__module__.split(".")[0] == "torch" and hasattr(image, "data_ptr"):
        import torch
        if image.dtype != torch.float32:
            raise ValueError("texture image must be float32, not %s" % image.dtype)
        image = np.ascontiguousarray(image.detach().cpu().numpy())
    if not isinstance(image, np.ndarray):
        raise ValueError("texture image must be a NumPy array or a torch tensor, not %s" % type(image).__name__)
    if image.dtype != np.float32:
        raise ValueError("texture image must be float32, not %s" % image.dtype)
    if image.ndim not in (2, 3) or (image.ndim == 3 and image.shape[2] not in (1, 3)):
        raise ValueError("texture image must have shape [yres, xres], [yres, xres, 1] or [yres, xres, 3], not %s" % (tuple(image.shape),))
    if not image.flags["C_CONTIGUOUS"]:
        raise ValueError("texture image must be C-contiguous (top row first)")
    return image, int(image.shape[1]), int(image.shape[0]), 1 if image.ndim == 2 else int(image.shape[2])


def scene_textures(scene):
    """The VspgSceneTextures record that travels with `scene` (created empty at first use): Renderer hands it to
    vspg_renderer_create_textured.  quad_texture[i] binds rectangle i: 0 = none, k = add_texture's return value."""
    if not hasattr(scene, "_textures"):
        scene._textures = VspgSceneTextures()
    return scene._textures


def add_texture(scene, image, filter="bilinear", wrap="repeat", scale=1.0, invert=False, uscale=1.0, vscale=1.0, udelta=0.0, vdelta=0.0):
    """One more image texture (`Texture "name" "spectrum" "imagemap"` under "uv" mapping): returns the value that binds it to a surface --
    scene_textures(scene).quad_texture[i] = that value, or set_triangle_textures' entries -- which is its index + 1 (0 = no texture).
    filter: "point" | "bilinear" ("trilinear" and "ewa" are bilinear at level 0); wrap: "repeat" | "clamp" | "black"."""
    filters = {"point": TEXFILTER_POINT, "bilinear": TEXFILTER_BILINEAR, "trilinear": TEXFILTER_BILINEAR, "ewa": TEXFILTER_BILINEAR}
    wraps = {"repeat": TEXWRAP_REPEAT, "clamp": TEXWRAP_CLAMP, "black": TEXWRAP_BLACK}
    img, xres, yres, channels = texture_image_source(image)
    tx = scene_textures(scene)
    k = tx.n_textures
    if k >= VSPG_MAX_TEXTURES:
        raise ValueError("a scene holds at most %d textures" % VSPG_MAX_TEXTURES)
    if isinstance(wrap, str) and wrap not in wraps:
        raise ValueError("texture wrap must be one of %s, not %r" % (sorted(wraps), wrap))
    if isinstance(filter, str) and filter not in filters:
        raise ValueError("texture filter must be one of %s, not %r" % (sorted(filters), filter))
    t = tx.textures[k]
    t.pixels = img.ctypes.data_as(C.POINTER(C.c_float))
    t.xres, t.yres, t.channels = xres, yres, channels
    t.wrap = wraps[wrap] if isinstance(wrap, str) else int(wrap)
    t.filter = filters[filter] if isinstance(filter, str) else int(filter)
    t.invert = 1 if invert else 0
    t.scale, t.su, t.sv, t.du, t.dv = scale, uscale, vscale, udelta, vdelta
    if not hasattr(scene, "_tex_keepalive"):
        scene._tex_keepalive = []
    scene._tex_keepalive.append(img)
    tx.n_textures = k + 1
    return k + 1


def set_triangle_textures(scene, tri_texture, tri_uv=None):
    """Bind textures to the scene's triangles (after set_triangles): tri_texture holds per triangle 0 (none) or add_texture's return
    value; tri_uv, if given, [n, 3, 2] per-vertex uv (else pbrt's default (0,0) (1,0) (1,1))."""
    import numpy as np
    tt = np.ascontiguousarray(tri_texture, dtype=np.int32).reshape(-1)
    if tt.shape[0] != scene.n_triangles:
        raise ValueError("tri_texture holds %d entries for %d triangles" % (tt.shape[0], scene.n_triangles))
    tx = scene_textures(scene)
    tx.tri_texture = tt.ctypes.data_as(C.POINTER(C.c_int32))
    keep = [tt]
    if tri_uv is not None:
        uv = np.ascontiguousarray(tri_uv, dtype=np.float32).reshape(-1, 6)
        if uv.shape[0] != scene.n_triangles:
            raise ValueError("tri_uv holds %d triangles' uv for %d triangles" % (uv.shape[0], scene.n_triangles))
        tx.tri_uv = uv.ctypes.data_as(C.POINTER(C.c_float))
        keep.append(uv)
    scene._tri_tex_keepalive = keep
    return scene


def app_f_params():
    """SURVEY.md App. F integrator line: primary-ray VSP guiding only."""
    p = default_params()
    p.surfaceguiding = 0
    p.volumeguiding = 0
    p.vspsecondaryguiding = 0
    return p


def environment_image_source(image, render_from_light=None):
    """What vspg_renderer_set_environment_image is handed: (image array, res, matrix array or None).  The image is a float32 NumPy array
    of shape [res, res, 3], C-contiguous, top row first, 1 <= res <= ENV_MAX_RES; the matrix, if any, 3 x 4 (or 12) numbers.  Anything
    else raises ValueError -- here, before the library is called."""
    import numpy as np
    if not isinstance(image, np.ndarray):
        raise ValueError("environment image must be a NumPy array, not %s" % type(image).__name__)
    if image.dtype != np.float32:
        raise ValueError("environment image must be float32, not %s" % image.dtype)
    if image.ndim != 3 or image.shape[2] != 3:
        raise ValueError("environment image must have shape [res, res, 3], not %s" % (tuple(image.shape),))
    if image.shape[0] != image.shape[1]:
        raise ValueError("environment image must be square (an equal-area map of the sphere), not %d x %d" % (image.shape[1], image.shape[0]))
    if not 1 <= image.shape[0] <= ENV_MAX_RES:
        raise ValueError("environment image resolution must be 1 .. %d, not %d" % (ENV_MAX_RES, image.shape[0]))
    if not image.flags["C_CONTIGUOUS"]:
        raise ValueError("environment image must be C-contiguous (top row first, R G B per texel)")
    m = None
    if render_from_light is not None:
        m = np.ascontiguousarray(render_from_light, dtype=np.float32)
        if m.size != 12:
            raise ValueError("render_from_light must be a 3 x 4 matrix, not %s" % (tuple(m.shape),))
        m = m.reshape(3, 4)
    return image, int(image.shape[0]), m


def portal_source(portal):
    """What vspg_renderer_set_portal_environment_image is handed for `portal`: a C-contiguous float32 array of the four vertices,
    [4, 3] (or 12 numbers), in render space.  Anything else raises ValueError -- here, before the library is called; the library
    judges the quadrilateral itself."""
    import numpy as np
    if portal is None:
        raise ValueError("portal must be four points (a [4, 3] array), not None")
    try:
        q = np.ascontiguousarray(portal, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError("portal must be four points (a [4, 3] array of numbers)")
    if q.size != 12:
        raise ValueError("portal must be four points (a [4, 3] array), not %s" % (tuple(q.shape),))
    return q.reshape(4, 3)


def grid_update_source(n_voxels, values, device):
    """What vspg_renderer_update_grid is handed for `values`: (address, memory kind, stream or None).  A NumPy array is a host source
    (float32, n_voxels elements, C-contiguous); a torch tensor is a device source (float32, n_voxels elements, contiguous, on
    cuda:`device`) whose stream is torch's current one.  Anything else raises ValueError -- here, before the library is called."""
    import numpy as np
    if isinstance(values, np.ndarray):
        if values.dtype != np.float32:
            raise ValueError("grid values must be float32, not %s" % values.dtype)
        if values.size != n_voxels:
            raise ValueError("grid values must hold nx*ny*nz = %d elements, not %d" % (n_voxels, values.size))
        if not values.flags["C_CONTIGUOUS"]:
            raise ValueError("grid values must be C-contiguous (x fastest)")
        return values.ctypes.data, MEM_HOST, None
    if type(values).__module__.split(".")[0] == "torch" and hasattr(values, "data_ptr"):
        import torch
        if values.dtype != torch.float32:
            raise ValueError("grid values must be float32, not %s" % values.dtype)
        if values.numel() != n_voxels:
            raise ValueError("grid values must hold nx*ny*nz = %d elements, not %d" % (n_voxels, values.numel()))
        if values.device.type != "cuda" or (values.device.index or 0) != device:
            raise ValueError("grid values must live on the renderer's device cuda:%d, not %s" % (device, values.device))
        if not values.is_contiguous():
            raise ValueError("grid values must be contiguous (x fastest)")
        return values.data_ptr(), MEM_DEVICE, torch.cuda.current_stream(values.device).cuda_stream
    raise ValueError("grid values must be a NumPy array or a torch tensor, not %s" % type(values).__name__)


def rgb_update_sources(n_voxels, sigma_a, sigma_s, Le, device):
    """What vspg_renderer_update_rgb_grids is handed: ([address or None] * 3, memory kind, stream or None).  Each given grid passes
    grid_update_source with 3 * n_voxels elements (R, G, B per voxel); None keeps a grid.  Raises ValueError -- here, before the
    library is called -- when nothing is given or when NumPy arrays and torch tensors are mixed (one memory kind per call)."""
    given = [g for g in (sigma_a, sigma_s, Le) if g is not None]
    if not given:
        raise ValueError("update_rgb needs at least one of sigma_a, sigma_s, Le")
    src = [None if g is None else grid_update_source(3 * n_voxels, g, device) for g in (sigma_a, sigma_s, Le)]
    kinds = {s[1] for s in src if s is not None}
    if len(kinds) != 1:
        raise ValueError("update_rgb takes NumPy arrays (host) or torch tensors (device), not both in one call")
    stream = next((s[2] for s in src if s is not None and s[2] is not None), None)
    return [None if s is None else s[0] for s in src], kinds.pop(), stream


class Renderer:
    """Thin RAII wrapper over the vspg_renderer_* entry points."""

    def __init__(self, scene, params, xres, yres, spp=1, seed=0, shard_index=0, shard_count=1, device=0):
        self.lib = load()
        self.cfg = VspgRenderConfig(xres, yres, spp, seed, shard_index, shard_count, device)
        self.scene, self.params = scene, params
        self.h = _vp()
        if hasattr(scene, "_textures"):   # image textures travel beside the scene (scene_textures)
            _check(self.lib, self.lib.vspg_renderer_create_textured(C.byref(scene), C.byref(scene._textures), C.byref(params), C.byref(self.cfg),
                                                                    C.byref(self.h)))
        else:
            _check(self.lib, self.lib.vspg_renderer_create(C.byref(scene), C.byref(params), C.byref(self.cfg),
                                                           C.byref(self.h)))
        self.xres, self.yres = xres, yres

    def close(self):
        if getattr(self, "h", None):
            self.lib.vspg_renderer_destroy(self.h)
            self.h = None

    __del__ = close

    def render_wave(self, w0, w1, stream=None):
        _check(self.lib, self.lib.vspg_render_wave(self.h, w0, w1, _vp(stream or 0)))

    def render_window(self, x0, y0, x1, y1, w0, w1, stream=None):
        """Sample indices [w0, w1) of the pixel window [x0, x1) x [y0, y1) (absolute film pixels, inside the frame) and of nothing
        else: every buffer keeps its full size.  render_wave(w0, w1) == render_window(0, 0, xres, yres, w0, w1)."""
        _check(self.lib, self.lib.vspg_render_window(self.h, int(x0), int(y0), int(x1), int(y1), w0, w1, _vp(stream or 0)))

    def isg_update_due(self, n_waves=1):
        return bool(self.lib.vspg_isg_update_due(self.h, int(n_waves)))

    def post_process_step(self, n_waves, isg_stats_sum_ptr=None, stream=None):
        """PostProcessWave after a step of n_waves sample indices; isg_stats_sum_ptr = device pointer (int) to the
        all-reduced statistics or None."""
        _check(self.lib, self.lib.vspg_post_process_step(self.h, int(n_waves), _vp(isg_stats_sum_ptr or 0), _vp(stream or 0)))

    def set_exchange(self, fn):
        """Sharded guiding-field training: fn(dev_ptr: int, n_floats: int, stream: int) sums the floats in place over the
        ranks (VspgExchangeFn); None removes the hook.  Exceptions in fn surface as an error of post_process_step."""
        if fn is None:
            self._exchange_cb = None
            _check(self.lib, self.lib.vspg_renderer_set_exchange(self.h, None, None))
            return

        def _cb(ptr, n, stream, _user):
            try:
                fn(int(ptr or 0), int(n), int(stream or 0))
                return 0
            except Exception:  # the C side turns a non-zero return into an error code
                import traceback
                traceback.print_exc()
                return VSPG_EHIP
        self._exchange_cb = EXCHANGE_FN(_cb)   # keep the thunk alive as long as the renderer may call it
        _check(self.lib, self.lib.vspg_renderer_set_exchange(self.h, C.cast(self._exchange_cb, _vp), None))

    def kernel_name(self):
        return (self.lib.vspg_renderer_kernel_name(self.h) or b"").decode()

    def set_arithmetic(self, mode):
        """ARITH_EXACT (default) / ARITH_FAST_WEIGHTS / ARITH_FAST (include/vspg.h, csrc/vspg_arith.h)."""
        _check(self.lib, self.lib.vspg_renderer_set_arithmetic(self.h, int(mode)))

    def arithmetic(self):
        return int(self.lib.vspg_renderer_get_arithmetic(self.h))

    def post_process_wave(self, stream=None):
        _check(self.lib, self.lib.vspg_post_process_wave(self.h, _vp(stream or 0)))

    def flush(self, stream=None):
        """Adds the samples the last one-sample wave parked to the film and the image-space statistics (asynchronous on
        `stream`): what a host that keeps film_ptr() / isg_stats_ptr() across waves calls before it reads through them."""
        _check(self.lib, self.lib.vspg_flush(self.h, _vp(stream or 0)))

    def film_ptr(self):
        p, n = _vp(), C.c_size_t()
        _check(self.lib, self.lib.vspg_film_device_ptr(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def isg_stats_ptr(self):
        p, n = _vp(), C.c_size_t()
        _check(self.lib, self.lib.vspg_isg_stats_device_ptr(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def vsp_ptr(self):
        p, n = _vp(), C.c_size_t()
        _check(self.lib, self.lib.vspg_vsp_buffer_device_ptr(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def film(self, stream=None):
        import numpy as np
        out = np.empty((self.yres, self.xres, 4), dtype=np.float32)
        _check(self.lib, self.lib.vspg_film_read(self.h, out.ctypes.data_as(_P(C.c_float)), _vp(stream or 0)))
        return out

    def film_clear(self, stream=None):
        _check(self.lib, self.lib.vspg_film_clear(self.h, _vp(stream or 0)))

    def set_reference_image(self, img, stream=None):
        """The reference image of the film-error records: (H, W, 3) float32, full frame, top row first; None removes it."""
        if img is None:
            _check(self.lib, self.lib.vspg_renderer_set_reference_image(self.h, None, _vp(stream or 0)))
            return
        import numpy as np
        v = np.ascontiguousarray(img, dtype=np.float32)
        if v.shape != (self.yres, self.xres, 3):
            raise ValueError("reference image has shape %r, the frame is %r" % (v.shape, (self.yres, self.xres, 3)))
        _check(self.lib, self.lib.vspg_renderer_set_reference_image(self.h, v.ctypes.data_as(_P(C.c_float)), _vp(stream or 0)))

    def film_error_enqueue(self, window=None, tag=0, stream=None):
        """Appends the error sums of the film as it stands over window = (x0, y0, x1, y1) (default: the frame) against the
        reference image to the device-side log: asynchronous on `stream`, no film read-back (vspg_film_error_enqueue)."""
        x0, y0, x1, y1 = window if window is not None else (0, 0, self.xres, self.yres)
        _check(self.lib, self.lib.vspg_film_error_enqueue(self.h, int(x0), int(y0), int(x1), int(y1), int(tag), _vp(stream or 0)))

    def film_errors(self, stream=None):
        """Synchronises `stream`, returns the log's records (FilmError) in enqueue order and empties the log."""
        buf = (VspgFilmError * FILM_ERROR_LOG_RECORDS)()
        n = C.c_size_t()
        _check(self.lib, self.lib.vspg_film_error_read(self.h, buf, FILM_ERROR_LOG_RECORDS, C.byref(n), _vp(stream or 0)))
        return [FilmError.from_c(buf[i]) for i in range(n.value)]

    def film_resolve(self, window=None, half=True, layout="rgb", stream=None):
        """The film's pixel values over window = (x0, y0, x1, y1) (default: the frame), resolved on the device (vspg_film_resolve):
        sum / weight per channel, for half=True clamped to the largest finite half and converted like the reference's Half(float).
        Returns (array, n_clamped): the array is float16 or float32, (h, w, 3) in R,G,B order for layout "rgb", (h, 3, w) in
        B,G,R order for layout "scanline" -- the payload of an OpenEXR scan-line block, row by row."""
        import numpy as np
        x0, y0, x1, y1 = (int(v) for v in (window if window is not None else (0, 0, self.xres, self.yres)))
        if layout not in ("rgb", "scanline"):
            raise ValueError("layout is %r: 'rgb' or 'scanline'" % (layout,))
        h, w = max(y1 - y0, 0), max(x1 - x0, 0)
        out = np.empty((h, w, 3) if layout == "rgb" else (h, 3, w), dtype=np.float16 if half else np.float32)
        n = C.c_uint64()
        _check(self.lib, self.lib.vspg_film_resolve(self.h, x0, y0, x1, y1, RESOLVE_F16 if half else RESOLVE_F32,
                                                    RESOLVE_RGB if layout == "rgb" else RESOLVE_SCANLINE_BGR,
                                                    out.ctypes.data_as(_vp), out.nbytes, C.byref(n), _vp(stream or 0)))
        return out, int(n.value)

    def vsp_buffer(self, stream=None):
        import numpy as np
        out = np.empty((self.yres, self.xres), dtype=np.float32)
        ready = C.c_int()
        _check(self.lib, self.lib.vspg_vsp_buffer_read(self.h, out.ctypes.data_as(_P(C.c_float)), C.byref(ready),
                                                      _vp(stream or 0)))
        return out, bool(ready.value)

    def load_vsp_buffer(self, vsp, stream=None):
        import numpy as np
        v = np.ascontiguousarray(vsp, dtype=np.float32)
        assert v.shape == (self.yres, self.xres)
        _check(self.lib, self.lib.vspg_vsp_buffer_load(self.h, v.ctypes.data_as(_P(C.c_float)), _vp(stream or 0)))

    def tr_buffer(self, stream=None):
        """TrBuffer read-back: (rgb (H, W, 3) float32, spp (H, W) int32)."""
        import numpy as np
        rgb = np.empty((self.yres, self.xres, 3), dtype=np.float32)
        spp = np.empty((self.yres, self.xres), dtype=np.int32)
        _check(self.lib, self.lib.vspg_renderer_get_tr_buffer(self.h, rgb.ctypes.data_as(_P(C.c_float)),
                                                             spp.ctypes.data_as(_P(C.c_int32)), _vp(stream or 0)))
        return rgb, spp

    def set_tr_buffer(self, rgb, stream=None):
        import numpy as np
        v = np.ascontiguousarray(rgb, dtype=np.float32)
        assert v.shape == (self.yres, self.xres, 3)
        _check(self.lib, self.lib.vspg_renderer_set_tr_buffer(self.h, v.ctypes.data_as(_P(C.c_float)), _vp(stream or 0)))

    def libm_powf_batch(self, x, y):
        import numpy as np
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.ascontiguousarray(y, dtype=np.float32)
        out = np.empty_like(x)
        fp = _P(C.c_float)
        _check(self.lib, self.lib.vspg_libm_powf_batch(self.h, x.shape[0], x.ctypes.data_as(fp), y.ctypes.data_as(fp),
                                                      out.ctypes.data_as(fp), _vp(0)))
        return out

    def blackbody_batch(self, u, T):
        """[n, 6]: SampleVisible(u)'s three wavelengths and BlackbodySpectrum(T).Sample at them, as the kernels evaluate them."""
        import numpy as np
        u = np.ascontiguousarray(u, dtype=np.float32)
        T = np.ascontiguousarray(T, dtype=np.float32)
        out = np.empty((u.shape[0], 6), dtype=np.float32)
        fp = _P(C.c_float)
        _check(self.lib, self.lib.vspg_blackbody_batch(self.h, u.shape[0], u.ctypes.data_as(fp), T.ctypes.data_as(fp),
                                                      out.ctypes.data_as(fp), _vp(0)))
        return out

    def set_environment_image(self, index, image, render_from_light=None, stream=None):
        """Give image infinite light `index` (of the scene's infinite lights) its image (vspg_renderer_set_environment_image): a
        float32 NumPy array [res, res, 3], top row first, an equal-area octahedral map of the sphere; render_from_light: 3 x 4 or
        None (identity).  Film, statistics, VSP buffer, guiding fields and counters stay."""
        img, res, m = environment_image_source(image, render_from_light)
        fp = _P(C.c_float)
        _check(self.lib, self.lib.vspg_renderer_set_environment_image(self.h, int(index), img.ctypes.data_as(fp), res,
                                                                     m.ctypes.data_as(fp) if m is not None else None, _vp(stream or 0)))

    def set_portal_environment_image(self, index, image, portal, render_from_light=None, stream=None):
        """Turn image infinite light `index` into a portal image infinite light (vspg_renderer_set_portal_environment_image): the
        image and matrix as set_environment_image takes them, portal: the opening's four vertices in render space, [4, 3].  The
        library refuses a quadrilateral that is no rectangle.  set_environment_image on the slot makes it a plain image light again.
        Film, statistics, VSP buffer, guiding fields and counters stay."""
        img, res, m = environment_image_source(image, render_from_light)
        q = portal_source(portal)
        fp = _P(C.c_float)
        _check(self.lib, self.lib.vspg_renderer_set_portal_environment_image(self.h, int(index), img.ctypes.data_as(fp), res,
                                                                            m.ctypes.data_as(fp) if m is not None else None,
                                                                            q.ctypes.data_as(fp), _vp(stream or 0)))

    def portallight_batch(self, index, ctx_p, dirs, u):
        """[n, 32] float32 per (context point, direction, variate pair) of portal light `index`, as the path kernels evaluate it
        (vspg_portallight_batch): bounds valid, bounds (4) | inside, uv (2), Le (3) | PDF_Li | sample valid, uv (2), mapPDF, duv_dw,
        wi (3), pdf, L (3) | trips x, trips y, why | pLight (3) | 0, 0."""
        import numpy as np
        p = np.ascontiguousarray(ctx_p, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        uu = np.ascontiguousarray(u, dtype=np.float32).reshape(-1, 2)
        if not p.shape[0] == d.shape[0] == uu.shape[0]:
            raise ValueError("portallight_batch: %d points, %d directions, %d variate pairs" % (p.shape[0], d.shape[0], uu.shape[0]))
        out = np.empty((p.shape[0], PORTALLIGHT_OUT), dtype=np.float32)
        fp = _P(C.c_float)
        _check(self.lib, self.lib.vspg_portallight_batch(self.h, int(index), p.shape[0], p.ctypes.data_as(fp), d.ctypes.data_as(fp),
                                                        uu.ctypes.data_as(fp), out.ctypes.data_as(fp), _vp(0)))
        return out

    def portallight_tables(self, index):
        """The tables of portal light `index` as the renderer holds them (vspg_portallight_read): a dict with res, image [res, res, 3],
        func [res, res], table [res, res] (the float summed-area table), p0, p2, frame [3, 3] (rows x, y, z), area, sum_phi (3), scene_radius."""
        import numpy as np
        res = C.c_int(0)
        rec = np.zeros(20, dtype=np.float32)
        fp = _P(C.c_float)
        _check(self.lib, self.lib.vspg_portallight_read(self.h, int(index), C.byref(res), None, None, None, rec.ctypes.data_as(fp), _vp(0)))
        n = res.value
        image, func, table = np.empty((n, n, 3), np.float32), np.empty((n, n), np.float32), np.empty((n, n), np.float32)
        _check(self.lib, self.lib.vspg_portallight_read(self.h, int(index), C.byref(res), image.ctypes.data_as(fp), func.ctypes.data_as(fp),
                                                       table.ctypes.data_as(fp), None, _vp(0)))
        return {"res": n, "image": image, "func": func, "table": table, "p0": rec[0:3].copy(), "p2": rec[3:6].copy(),
                "frame": rec[6:15].reshape(3, 3).copy(), "area": rec[15], "sum_phi": rec[16:19].copy(), "scene_radius": rec[19]}

    def set_light_image(self, index, image, stream=None):
        """Give the projection or goniometric light in point-light slot `index` its image (vspg_renderer_set_light_image): a float32
        NumPy array, top row first -- [yres, xres, 3] (R, G, B) for a projection light, [res, res] or [res, res, 1] (Y) for a
        goniometric light.  The library judges everything else (the slot's type, the channels, the resolution, the pixel values).
        Film, statistics, VSP buffer, guiding fields and counters stay."""
        import numpy as np
        if not isinstance(image, np.ndarray) or image.dtype != np.float32 or image.ndim not in (2, 3) or not image.flags["C_CONTIGUOUS"]:
            raise ValueError("light image must be a C-contiguous float32 NumPy array [yres, xres] or [yres, xres, channels]")
        channels = 1 if image.ndim == 2 else int(image.shape[2])
        _check(self.lib, self.lib.vspg_renderer_set_light_image(self.h, int(index), image.ctypes.data_as(_P(C.c_float)), int(image.shape[1]),
                                                               int(image.shape[0]), channels, _vp(stream or 0)))

    def set_texture_image(self, index, image, stream=None):
        """Replace the image of texture `index` (0-based) on the live renderer (vspg_renderer_set_texture_image): a float32 NumPy
        array or torch tensor [yres, xres], [yres, xres, 1] or [yres, xres, 3], top row first (texture_image_source).  The resolution
        and the channel count may change; the texture's other parameters stay, and so do film, statistics, VSP buffer, guiding fields
        and counters."""
        img, xres, yres, channels = texture_image_source(image)
        _check(self.lib, self.lib.vspg_renderer_set_texture_image(self.h, int(index), img.ctypes.data_as(_P(C.c_float)), xres, yres, channels,
                                                                 _vp(stream or 0)))

    def set_camera(self, cam, model=0, lens_radius=0.0, focal_distance=1e6, stream=None):
        """Replace the camera of the live renderer (vspg_renderer_set_camera): a VspgCamera (camera_look_at_window) and the model
        CAMERA_* with its thin lens; model=None passes a null record (the pinhole perspective).  Nothing is cleared: film, statistics
        and buffers keep what they gathered under the old camera."""
        m = None if model is None else C.byref(VspgCameraModel(int(model), float(lens_radius), float(focal_distance)))
        _check(self.lib, self.lib.vspg_renderer_set_camera(self.h, C.byref(cam), m, _vp(stream or 0)))

    def camera_ray_batch(self, pixel_xy, sample_index, u=None):
        """The render-space camera ray (origins [n, 3], directions [n, 3]) of sample sample_index[i] of pixel pixel_xy[i], as the path
        kernels generate it (vspg_camera_ray_batch).  u: [n, 4] filter and lens variates, or None = the renderer's own sampler."""
        import numpy as np
        pix = np.ascontiguousarray(pixel_xy, dtype=np.int32).reshape(-1, 2)
        si = np.ascontiguousarray(sample_index, dtype=np.int32).reshape(-1)
        n = si.shape[0]
        if pix.shape[0] != n:
            raise ValueError("camera_ray_batch: %d pixels but %d sample indices" % (pix.shape[0], n))
        fp = _P(C.c_float)
        uu = None
        if u is not None:
            uu = np.ascontiguousarray(u, dtype=np.float32).reshape(-1, 4)
            if uu.shape[0] != n:
                raise ValueError("camera_ray_batch: %d pixels but %d variate rows" % (n, uu.shape[0]))
        o, d = np.empty((n, 3), dtype=np.float32), np.empty((n, 3), dtype=np.float32)
        _check(self.lib, self.lib.vspg_camera_ray_batch(self.h, n, pix.ctypes.data_as(_P(C.c_int32)), si.ctypes.data_as(_P(C.c_int32)),
                                                       None if uu is None else uu.ctypes.data_as(fp), o.ctypes.data_as(fp), d.ctypes.data_as(fp), None))
        return o, d

    def texture_eval_batch(self, prim, hit):
        """Per (primitive, three floats of a vertex): (u, v), (s, t) after the flip, R (3) and has_lobes, as the path kernels evaluate
        them (vspg_texture_eval_batch).  prim: a rectangle's index or -2 - j for triangle j; hit: the point on the rectangle or the
        triangle hit's barycentrics.  Returns an (n, TEXTURE_EVAL_OUT) float32 array."""
        import numpy as np
        pr = np.ascontiguousarray(np.asarray(prim, dtype=np.int32).reshape(-1))
        h = np.ascontiguousarray(np.asarray(hit, dtype=np.float32).reshape(-1, 3))
        if pr.shape[0] != h.shape[0]:
            raise ValueError("texture_eval_batch: %d primitives but %d hits" % (pr.shape[0], h.shape[0]))
        out = np.empty((pr.shape[0], TEXTURE_EVAL_OUT), dtype=np.float32)
        _check(self.lib, self.lib.vspg_texture_eval_batch(self.h, pr.shape[0], pr.ctypes.data_as(_P(C.c_int32)), h.ctypes.data_as(_P(C.c_float)),
                                                         out.ctypes.data_as(_P(C.c_float)), None))
        return out

    def envlight_batch(self, index, dirs, u):
        """[n, 16] float32 per (direction, variate pair): Le (3), its uv (2), PDF_Li, then SampleLi(u): valid, uv (2), wi (3), pdf,
        L (3) of image infinite light `index`, as the path kernels evaluate them (vspg_envlight_batch)."""
        import numpy as np
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        uu = np.ascontiguousarray(u, dtype=np.float32).reshape(-1, 2)
        if d.shape[0] != uu.shape[0]:
            raise ValueError("envlight_batch: %d directions but %d variate pairs" % (d.shape[0], uu.shape[0]))
        out = np.empty((d.shape[0], ENVLIGHT_OUT), dtype=np.float32)
        fp = _P(C.c_float)
        _check(self.lib, self.lib.vspg_envlight_batch(self.h, int(index), d.shape[0], d.ctypes.data_as(fp), uu.ctypes.data_as(fp),
                                                     out.ctypes.data_as(fp), _vp(0)))
        return out

    def light_sample_batch(self, ctx_p, ctx_n, u):
        """Per context (point ctx_p, normal ctx_n -- zeros = a medium vertex) and variates u = (pick, u0, u1): the light the renderer's
        light sampler picks and that light's SampleLi, as the path kernels evaluate them (vspg_light_sample_batch).  Returns an
        (n, LIGHT_SAMPLE_OUT) float32 array: index | pmf | PMF(ctx, light) | has sample | wi (3) | L (3) | pdf | pLight (3) | delta | 0."""
        import numpy as np
        p = np.ascontiguousarray(np.asarray(ctx_p, dtype=np.float32).reshape(-1, 3))
        nn = np.ascontiguousarray(np.asarray(ctx_n, dtype=np.float32).reshape(-1, 3))
        uu = np.ascontiguousarray(np.asarray(u, dtype=np.float32).reshape(-1, 3))
        if not (p.shape[0] == nn.shape[0] == uu.shape[0]):
            raise ValueError("light_sample_batch: %d points, %d normals, %d variate triples" % (p.shape[0], nn.shape[0], uu.shape[0]))
        out = np.empty((p.shape[0], LIGHT_SAMPLE_OUT), dtype=np.float32)
        fp = C.POINTER(C.c_float)
        _check(self.lib, self.lib.vspg_light_sample_batch(self.h, p.shape[0], p.ctypes.data_as(fp), nn.ctypes.data_as(fp), uu.ctypes.data_as(fp),
                                                          out.ctypes.data_as(fp), None))
        return out

    def light_pdf_batch(self, light_index, ctx_p, ctx_n, wi, ctx_perr=None):
        """Per context (point ctx_p, optional error bounds ctx_perr, normal ctx_n -- zeros = a medium vertex) and direction wi: what the path
        kernels compute when the ray from the context along wi is weighed against light `light_index` (a rectangle or a sphere of the
        light list; vspg_light_pdf_batch).  Returns an (n, LIGHT_PDF_OUT) float32 array: PDF_Li | PMF(ctx, light) | hit | L (3) | t | 0."""
        import numpy as np
        fp = C.POINTER(C.c_float)
        arrs = [np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, 3)) for a in (ctx_p, ctx_n, wi)]
        e = None if ctx_perr is None else np.ascontiguousarray(np.asarray(ctx_perr, dtype=np.float32).reshape(-1, 3))
        n = arrs[0].shape[0]
        if any(a.shape[0] != n for a in arrs) or (e is not None and e.shape[0] != n):
            raise ValueError("light_pdf_batch: arrays of different lengths")
        out = np.empty((n, LIGHT_PDF_OUT), dtype=np.float32)
        _check(self.lib, self.lib.vspg_light_pdf_batch(self.h, int(light_index), n, arrs[0].ctypes.data_as(fp), None if e is None else e.ctypes.data_as(fp),
                                                       arrs[1].ctypes.data_as(fp), arrs[2].ctypes.data_as(fp), out.ctypes.data_as(fp), None))
        return out

    def counters(self, stream=None):
        c = VspgCounters()
        _check(self.lib, self.lib.vspg_get_counters(self.h, C.byref(c), _vp(stream or 0)))
        return c.as_dict()

    def reset_counters(self, stream=None):
        _check(self.lib, self.lib.vspg_reset_counters(self.h, _vp(stream or 0)))

    def trace_paths(self, pixel_xy, sample_index):
        import numpy as np
        pix = np.ascontiguousarray(pixel_xy, dtype=np.int32).reshape(-1, 2)
        si = np.ascontiguousarray(sample_index, dtype=np.int32).reshape(-1)
        n = si.shape[0]
        L = np.empty((n, 3), dtype=np.float32)
        seg = np.empty(n, dtype=np.int32)
        _check(self.lib, self.lib.vspg_trace_paths(self.h, n, pix.ctypes.data_as(_P(C.c_int32)),
                                                   si.ctypes.data_as(_P(C.c_int32)),
                                                   L.ctypes.data_as(_P(C.c_float)),
                                                   seg.ctypes.data_as(_P(C.c_int32)), _vp(0)))
        return L, seg

    def ray_batch(self, queries):
        """queries: numpy structured array of RAY_QUERY_DTYPE; returns one of RAY_RESULT_DTYPE (vspg_ray_batch)."""
        import numpy as np
        q = np.ascontiguousarray(queries, dtype=RAY_QUERY_DTYPE)
        out = np.zeros(len(q), dtype=RAY_RESULT_DTYPE)
        assert q.itemsize == C.sizeof(VspgRayQuery) and out.itemsize == C.sizeof(VspgRayResult)
        _check(self.lib, self.lib.vspg_ray_batch(self.h, len(q), q.ctypes.data_as(_P(VspgRayQuery)), out.ctypes.data_as(_P(VspgRayResult)), None))
        return out

    def sample_tmaj_batch(self, variant, queries):
        n = len(queries)
        q = (VspgTmajQuery * n)(*queries)
        out = (VspgTmajResult * n)()
        _check(self.lib, self.lib.vspg_sample_tmaj_batch(self.h, variant, n, q, out, _vp(0)))
        return list(out)

    def brick_info(self):
        """The device layout of a grid medium's density (vspg_brick_info): dict with bnx, bny, bnz, indexed, n_stored,
        index_bytes, octet_bytes."""
        bi = VspgBrickInfo()
        _check(self.lib, self.lib.vspg_brick_info(self.h, C.byref(bi)))
        return {k: int(getattr(bi, k)) for k, _ in VspgBrickInfo._fields_}

    def brick_storage(self, index=True, octets=True):
        """(index [bnz, bny, bnx] int32 -- slot or -1, the identity when every brick is stored --, octets
        [n_stored, 8, 8, 8, 8] float32 -- brick, z, y, x in the brick, corner) as the kernels read them (vspg_brick_read)."""
        import numpy as np
        bi = self.brick_info()
        idx = np.empty((bi["bnz"], bi["bny"], bi["bnx"]), dtype=np.int32) if index else None
        octs = np.empty((bi["n_stored"], 8, 8, 8, 8), dtype=np.float32) if octets else None
        _check(self.lib, self.lib.vspg_brick_read(self.h, idx.ctypes.data_as(_P(C.c_int32)) if index else None,
                                                 octs.ctypes.data_as(_P(C.c_float)) if octets else None, _vp(0)))
        return idx, octs

    def _update_grid(self, which, values, stream):
        m = self.scene.medium
        n = int(m.nx) * int(m.ny) * int(m.nz)
        ptr, memory, cur = grid_update_source(n, values, int(self.cfg.device))
        if stream is None:
            stream = cur  # (a device source: torch's current stream, the one its producer ran on)
        _check(self.lib, self.lib.vspg_renderer_update_grid(self.h, which, _vp(ptr), n, memory, _vp(stream or 0)))

    def update_density(self, values, stream=None):
        """Replace the density grid's values in place (vspg_renderer_update_grid): a float32 NumPy array (host path) or a float32
        torch tensor on the renderer's device (device path, read where it lies), nx*ny*nz elements, x fastest.  Majorants and
        bricks are rebuilt; film, statistics, VSP buffer, guiding fields and counters stay."""
        self._update_grid(GRID_DENSITY, values, stream)

    def update_temperature(self, values, stream=None):
        """Replace the temperature grid's values (a renderer created with one), as update_density takes them."""
        self._update_grid(GRID_TEMPERATURE, values, stream)

    def update_rgb(self, sigma_a=None, sigma_s=None, Le=None, stream=None):
        """Replace an RGB grid medium's sigma_a / sigma_s / Le values in place (vspg_renderer_update_rgb_grids): float32 NumPy arrays
        (host path) or float32 torch tensors on the renderer's device (device path, read where they lie), 3*nx*ny*nz elements each,
        R, G, B per voxel, x fastest; None keeps a grid.  Octets and majorants are rebuilt on the device; film, statistics, VSP
        buffer, guiding fields and counters stay."""
        m = self.scene.medium
        n = int(m.nx) * int(m.ny) * int(m.nz)
        ptrs, memory, cur = rgb_update_sources(n, sigma_a, sigma_s, Le, int(self.cfg.device))
        if stream is None:
            stream = cur  # (a device source: torch's current stream, the one its producer ran on)
        _check(self.lib, self.lib.vspg_renderer_update_rgb_grids(self.h, _vp(ptrs[0]), _vp(ptrs[1]), _vp(ptrs[2]), 3 * n, memory, _vp(stream or 0)))

    def rgb_octets(self, which):
        """The device image of an RGB grid medium's sigma_a (which = 0) or sigma_s (1) grid (vspg_rgb_octets_read):
        [bnz, bny, bnx, 8, 8, 8, 8, 4] float32 -- brick z, y, x; octet z, y, x in the brick; corner; R, G, B, 0."""
        import numpy as np
        m = self.scene.medium
        bn = [(int(v) + 8) // 8 for v in (m.nx, m.ny, m.nz)]
        out = np.empty((bn[2], bn[1], bn[0], 8, 8, 8, 8, 4), dtype=np.float32)
        _check(self.lib, self.lib.vspg_rgb_octets_read(self.h, int(which), out.ctypes.data_as(_P(C.c_float)), out.size, _vp(0)))
        return out

    def majorant(self, stream=None):
        """The majorant grid the kernels read (vspg_majorant_read): [R, R, R] float32 indexed z, y, x; R = 16 (GRID, RGBGRID) or 64 (NANOVDB)."""
        import numpy as np
        R = 64 if self.scene.medium.type == MEDIUM_NANOVDB else 16
        out = np.empty((R, R, R), dtype=np.float32)
        res = C.c_int32(0)
        _check(self.lib, self.lib.vspg_majorant_read(self.h, out.ctypes.data_as(_P(C.c_float)), out.size, C.byref(res), _vp(stream or 0)))
        assert res.value == R
        return out

    def medium_point_batch(self, p):
        """[n, 10] float32 per render-space point of p [n, 3]: sigma_a, sigma_s, Le (3 each) of SamplePoint(p) and the value of the
        majorant cell that holds p, 0 outside the bounds (vspg_medium_point_batch); grid media."""
        import numpy as np
        p = np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 3)
        out = np.zeros((len(p), MEDIUM_POINT_OUT), dtype=np.float32)
        _check(self.lib, self.lib.vspg_medium_point_batch(self.h, len(p), p.ctypes.data_as(_P(C.c_float)), out.ctypes.data_as(_P(C.c_float)), _vp(0)))
        return out

    def primitives_batch(self, f, g):
        import numpy as np
        f = np.ascontiguousarray(f, dtype=np.float32)
        g = np.ascontiguousarray(g, dtype=np.float32)
        n = f.shape[0]
        h = np.empty(n, dtype=np.uint64)
        r = np.empty(n, dtype=np.uint32)
        e = np.empty(n, dtype=np.float32)
        _check(self.lib, self.lib.vspg_primitives_batch(self.h, n, f.ctypes.data_as(_P(C.c_float)),
                                                        g.ctypes.data_as(_P(C.c_float)),
                                                        h.ctypes.data_as(_P(C.c_uint64)),
                                                        r.ctypes.data_as(_P(C.c_uint32)),
                                                        e.ctypes.data_as(_P(C.c_float)), _vp(0)))
        return h, r, e

    def libm_batch(self, x):
        import numpy as np
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = x.shape[0]
        lo, so, co = (np.empty(n, dtype=np.float32) for _ in range(3))
        fp = _P(C.c_float)
        _check(self.lib, self.lib.vspg_libm_batch(self.h, n, x.ctypes.data_as(fp), lo.ctypes.data_as(fp),
                                                  so.ctypes.data_as(fp), co.ctypes.data_as(fp), _vp(0)))
        return lo, so, co

    # ---- guiding-cache training (a18)
    def training_stats(self):
        st = VspgTrainStats()
        _check(self.lib, self.lib.vspg_renderer_training_stats(self.h, C.byref(st), _vp(0)))
        return st.as_dict()

    def train_samples(self):
        import numpy as np
        n = C.c_size_t(0)
        _check(self.lib, self.lib.vspg_train_samples_read(self.h, None, 0, C.byref(n), _vp(0)))
        buf = (VspgTrainSample * max(1, n.value))()
        _check(self.lib, self.lib.vspg_train_samples_read(self.h, buf, n.value, C.byref(n), _vp(0)))
        return np.frombuffer(buf, dtype=TRAIN_SAMPLE_DTYPE, count=n.value).copy()

    def get_guiding_field(self, volume):
        nn, nr = C.c_int32(0), C.c_int32(0)
        _check(self.lib, self.lib.vspg_renderer_get_guiding_field(self.h, int(volume), None, None, C.byref(nn), C.byref(nr), _vp(0)))
        nodes = (VspgKdNode * max(1, nn.value))()
        regs = (VspgFieldRegion * max(1, nr.value))()
        _check(self.lib, self.lib.vspg_renderer_get_guiding_field(self.h, int(volume), nodes, regs, C.byref(nn), C.byref(nr), _vp(0)))
        return nodes, regs, nn.value, nr.value

    def libm_log1m_batch(self, x):
        import numpy as np
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty_like(x)
        fp = _P(C.c_float)
        _check(self.lib, self.lib.vspg_libm_log1m_batch(self.h, x.shape[0], x.ctypes.data_as(fp), out.ctypes.data_as(fp), _vp(0)))
        return out

    def set_guiding_field(self, surface, volume, stream=None):
        _check(self.lib, self.lib.vspg_renderer_set_guiding_field(self.h, C.byref(surface.pod) if surface else None,
                                                                  C.byref(volume.pod) if volume else None, _vp(stream or 0)))


def _guiding_query(self, is_volume, g, p, n_or_wo, wi, u):
    import numpy as np
    fp = _P(C.c_float)
    p, a, wi, u = (np.ascontiguousarray(x, dtype=np.float32) for x in (p, n_or_wo, wi, u))
    n = p.shape[0]
    ok = np.zeros(n, dtype=np.int32)
    pdf, inc, vsp, pdfs = (np.zeros(n, dtype=np.float32) for _ in range(4))
    ws = np.zeros((n, 3), dtype=np.float32)
    _check(self.lib, self.lib.vspg_guiding_query_batch(self.h, int(is_volume), float(g), n, p.ctypes.data_as(fp),
                                                       a.ctypes.data_as(fp), wi.ctypes.data_as(fp), u.ctypes.data_as(fp),
                                                       ok.ctypes.data_as(_P(C.c_int32)), pdf.ctypes.data_as(fp),
                                                       inc.ctypes.data_as(fp), vsp.ctypes.data_as(fp), ws.ctypes.data_as(fp),
                                                       pdfs.ctypes.data_as(fp), _vp(0)))
    return dict(ok=ok, pdf=pdf, incoming_pdf=inc, vsp=vsp, ws=ws, pdf_s=pdfs)


Renderer.guiding_query_batch = _guiding_query


class Field:
    """Host-side container of a guiding field (kd-tree nodes + regions) keeping the arrays alive."""

    def __init__(self, nodes, regions):
        self.nodes = (VspgKdNode * len(nodes))(*nodes)
        self.regions = (VspgFieldRegion * len(regions))(*regions)
        self.pod = VspgField(len(nodes), len(regions), self.nodes, self.regions)
