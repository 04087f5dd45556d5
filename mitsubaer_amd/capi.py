"""ctypes binding of libmer.so (include/mer.h): the HIP hot path.  No CPU fallback exists --
loading fails loudly if the library is missing, and context creation fails without a GPU."""
import collections
import ctypes as C
import os
from types import SimpleNamespace
import numpy as np
from . import params as P

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MER_LIB", os.path.join(_HERE, "libmer.so"))
CHECK_LIB_PATH = os.path.join(_HERE, "libmer_check.so")     # same sources, -DMER_BOUNDS_CHECK (Context(check=True))
_LIBS = {}

C_PATHS, C_STEPS, C_RIF_EVALS, C_TENTATIVE, C_REAL, C_SEGMENTS, C_NEE, C_LOOP_ITERS, C_ACTIVE_LANES, C_CONNECT_UNITS, C_CONNECT_STEPS, C_CONNECT_LANE_SLOTS, C_SIDE_SPAWNED, C_SIDE_INLINE = range(14)
C_COUNT = 16
LAYOUT_DENSE, LAYOUT_CELL8, LAYOUT_BRICK27, LAYOUT_BRICK125, LAYOUT_AUTO = 0, 1, 2, 3, 4

# every symbol include/mer.h declares (checked by tests/test_abi.py against the header text)
SYMBOLS = [
    "mer_abi_version", "mer_context_create", "mer_context_destroy", "mer_last_error", "mer_context_set_stream",
    "mer_device_info", "mer_context_set_option", "mer_context_get_option", "mer_debug_bounds", "mer_volume_upload", "mer_volume_upload_dev", "mer_sdf_from_mesh", "mer_volume_download", "mer_volume_build_spline",
    "mer_volume_download_spline", "mer_volume_destroy", "mer_film_channels", "mer_film_alloc_n", "mer_film_zero_n",
    "mer_film_download_n", "mer_film_alloc", "mer_film_zero", "mer_film_download",
    "mer_film_free", "mer_render", "mer_synchronize", "mer_last_kernel_ms", "mer_last_render_stats", "mer_counters_read",
    "mer_counters_reset", "mer_lookup_trilinear", "mer_lookup_trilinear_rgb", "mer_rif_value_grad", "mer_acoustic_value_grad", "mer_er_trace",
    "mer_sample_distance", "mer_connect", "mer_emitter_direct", "mer_area_direct", "mer_area_hit", "mer_envmap_upload", "mer_envmap_eval", "mer_envmap_sample", "mer_multi_envmap_upload", "mer_eval_transmittance", "mer_phase_sample", "mer_phase_eval", "mer_rough_dielectric_eval",
    "mer_rough_dielectric_sample", "mer_camera_rays", "mer_sensor_rays", "mer_sensor_direct", "mer_sensor_position",
    "mer_correlation", "mer_render_paths", "mer_rng_floats", "mer_synth_field_dev", "mer_device_free",
    "mer_multi_create", "mer_multi_destroy", "mer_multi_last_error", "mer_multi_size", "mer_multi_context", "mer_multi_set_option",
    "mer_multi_volume_upload", "mer_multi_volume_build_spline", "mer_multi_volume_destroy", "mer_multi_render", "mer_multi_last_stats",
    "mer_fluence_create", "mer_fluence_clear", "mer_fluence_destroy", "mer_render_fluence", "mer_fluence_read",
    "mer_fluence_time_create", "mer_fluence_time_read", "mer_fluence_track_create",
    "mer_exitance_create", "mer_exitance_clear", "mer_exitance_destroy", "mer_render_exitance", "mer_exitance_read",
    "mer_fluence_fd_create", "mer_fluence_fd_read", "mer_exitance_fd_create", "mer_exitance_fd_read",
    "mer_sensitivity_create", "mer_sensitivity_clear", "mer_sensitivity_destroy", "mer_render_sensitivity", "mer_sensitivity_read",
    "mer_sensitivity_array_create", "mer_sensitivity_shape", "mer_sensitivity_read_array",
]
SHARD_SAMPLES, SHARD_TILES = 0, 1
REDUCE_NONE, REDUCE_RCCL, REDUCE_PEER_COPY = 0, 1, 2


class GridDesc(C.Structure):
    _fields_ = [("res", C.c_int32 * 3), ("channels", C.c_int32), ("dtype", C.c_int32),
                ("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3), ("world_to_volume", C.c_float * 12)]


class _SpotAngles(C.Structure):
    _fields_ = [("cutoff_angle_deg", C.c_float), ("beam_width_deg", C.c_float), ("spot_reserved", C.c_float)]


class _EnvmapRef(C.Structure):
    _fields_ = [("envmap", C.c_int32), ("env_scale", C.c_float), ("env_reserved", C.c_float)]


class _RadianceOrAngles(C.Union):
    _anonymous_ = ("_angles", "_env")
    _fields_ = [("radiance", C.c_float * 3), ("_angles", _SpotAngles), ("_env", _EnvmapRef)]


class EmitterDesc(C.Structure):
    """mer_emitter: one entry of SceneDesc.emitters (a spot's cutoff_angle_deg / beam_width_deg and an envmap's envmap / env_scale overlay radiance)"""
    _anonymous_ = ("_u",)
    _fields_ = [("type", C.c_int32), ("position", C.c_float * 3), ("intensity", C.c_float * 3),
                ("to_world", C.c_float * 12), ("_u", _RadianceOrAngles), ("sampling_weight", C.c_float)]


class SceneDesc(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("fov_x_deg", C.c_float), ("near_clip", C.c_float), ("far_clip", C.c_float),
        ("cam_to_world", C.c_float * 12),
        ("rfilter", C.c_int32), ("rfilter_param", C.c_float),
        ("max_depth", C.c_int32), ("rr_depth", C.c_int32), ("hide_emitters", C.c_int32),
        ("boundary", C.c_int32), ("bmin", C.c_float * 3), ("bmax", C.c_float * 3),
        ("sph_center", C.c_float * 3), ("sph_radius", C.c_float),
        ("sigma_mode", C.c_int32), ("sigma_a", C.c_float * 3), ("sigma_s", C.c_float * 3),
        ("strategy", C.c_int32), ("channel", C.c_int32), ("sampling_density", C.c_float),
        ("medium_sampling_weight", C.c_float),
        ("density", C.c_int32), ("density_scale", C.c_float),
        ("albedo_mode", C.c_int32), ("albedo", C.c_float * 3), ("albedo_grid", C.c_int32),
        ("rif_mode", C.c_int32), ("rif_const", C.c_float), ("rif", C.c_int32),
        ("stepper", C.c_int32), ("stepsize", C.c_float),
        ("phase", C.c_int32), ("g", C.c_float),
        ("tr_estimator", C.c_int32),
        ("env_radiance", C.c_float * 3), ("emission", C.c_float * 3),
        ("point_position", C.c_float * 3), ("point_intensity", C.c_float * 3),
        ("decomposition", C.c_int32), ("min_bound", C.c_float), ("max_bound", C.c_float), ("bin_width", C.c_float),
        ("calibrated_transient", C.c_int32),
        ("modulation", C.c_int32), ("mod_lambda", C.c_float), ("mod_phase_deg", C.c_float), ("mod_P", C.c_int32), ("mod_neighbors", C.c_int32),
        ("boundary_bsdf", C.c_int32),
        ("sdf", C.c_int32),
        ("aggressive_tracing", C.c_int32),
        ("sdf_max_error", C.c_float),
        ("ac_n_o", C.c_float), ("ac_n_max", C.c_float), ("ac_k_r", C.c_float), ("ac_mode", C.c_int32),
        ("method", C.c_int32), ("het_stepsize", C.c_float),
        ("area_to_world", C.c_float * 12), ("area_radiance", C.c_float * 3),
        ("integrator", C.c_int32), ("integrator_reserved", C.c_int32),
        ("emitters", C.POINTER(EmitterDesc)), ("n_emitters", C.c_int32),
        ("sensor", C.c_int32), ("aperture_radius", C.c_float), ("focus_distance", C.c_float), ("sensor_reserved", C.c_int32),
        ("rough_distribution", C.c_int32), ("rough_alpha", C.c_float), ("rough_sample_visible", C.c_int32),
    ]


def _rows3x4(to_world):
    """a 3x4 / 4x4 transform (None = identity) as the 12 row-major float32 values of the C structs"""
    m = np.eye(4); t = np.asarray(to_world if to_world is not None else np.eye(4), np.float64); m[:t.shape[0], :4] = t
    return [float(v) for v in m[:3, :4].astype(np.float32).reshape(-1)]


def _sdf_value(p, x):
    """the signed-distance grid of p at the world point x (trilinear, as the kernels look it up); off the grid: +inf (outside)"""
    g = np.asarray(p.sdf, np.float64)
    if g.ndim == 4:
        g = g[..., 0]
    if p.sdf_to_world is not None:
        m = P.world_to_volume(p.sdf_to_world).astype(np.float64)
        x = m[:, :3] @ x + m[:, 3]
    lo, hi = np.asarray(p.sdf_aabb[0], np.float64), np.asarray(p.sdf_aabb[1], np.float64)
    res = np.array(g.shape[::-1])                         # grids are [z][y][x]
    c = (x - lo) * (res - 1) / (hi - lo)
    i = np.floor(c).astype(int)
    if np.any(i < 0) or np.any(i >= res - 1):
        return np.inf
    f = c - i
    v = 0.0
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                w = (f[0] if dx else 1 - f[0]) * (f[1] if dy else 1 - f[1]) * (f[2] if dz else 1 - f[2])
                v += w * g[i[2] + dz, i[1] + dy, i[0] + dx]
    return v


def validate_sensor(p):
    """The refusals of the sensor fields (mer_render / the host parser): MerError.  No GPU needed."""
    if p.sensor not in (P.SENSOR_PERSPECTIVE, P.SENSOR_ORTHOGRAPHIC, P.SENSOR_THINLENS, P.SENSOR_TELECENTRIC):
        raise MerError("sensor: unknown sensor kind (perspective, orthographic, thinlens, telecentric)")
    if p.sensor == P.SENSOR_PERSPECTIVE:
        return
    m = np.asarray(p.cam_to_world, np.float64)[:3, :3]
    if not (np.all(np.isfinite(np.asarray(p.cam_to_world, np.float64))) and abs(np.linalg.det(m)) > 1e-12):
        raise MerError("sensor: cam_to_world is singular")
    if p.sensor == P.SENSOR_ORTHOGRAPHIC:
        return
    if not (np.isfinite(p.aperture_radius) and p.aperture_radius >= 0):
        raise MerError("sensor: aperture_radius must be finite and non-negative")
    if not (np.isfinite(p.focus_distance) and p.focus_distance > 0):
        raise MerError("sensor: focus_distance must be finite and positive")


def validate_rough(p):
    """The refusals of a rough dielectric boundary (mer_render / the host parser): MerError.  No GPU needed."""
    if p.boundary_bsdf not in (P.BSDF_NULL, P.BSDF_HDIELECTRIC, P.BSDF_HROUGHDIELECTRIC):
        raise MerError("boundary BSDF must be null, hdielectric or hroughdielectric")
    if p.boundary_bsdf != P.BSDF_HROUGHDIELECTRIC:
        return
    if p.rough_distribution not in (P.MICROFACET_BECKMANN, P.MICROFACET_GGX, P.MICROFACET_PHONG):
        raise MerError("hroughdielectric: distribution must be beckmann, ggx or phong")
    if not (np.isfinite(p.rough_alpha) and p.rough_alpha >= 0):
        raise MerError("hroughdielectric: alpha must be finite and >= 0")
    if any(v != 0 for v in p.area_radiance):
        raise MerError("hroughdielectric: the area emitter needs an index-matched (null) boundary")
    if any(v != 0 for v in p.point_intensity):
        x = np.asarray(p.point_position, np.float64)
        if p.boundary == P.BOUNDARY_AABB:
            inside = bool(np.all(x >= np.asarray(p.bmin)) and np.all(x <= np.asarray(p.bmax)))
        elif p.boundary == P.BOUNDARY_SPHERE:
            inside = float(np.sum((x - np.asarray(p.sph_center)) ** 2)) < p.sph_radius ** 2
        elif p.sdf is not None:
            inside = _sdf_value(p, x) < 0
        else:
            inside = False
        if inside:
            raise MerError("hroughdielectric: the point emitter must lie outside the medium shape "
                           "(a curved connection that starts on the boundary is not built)")


def _rect_meets_shape(p, m):
    """exact test that the rectangle O + a U + b V (a, b in [-1, 1]; columns of the 3x4 m) meets the closed cube / sphere of p"""
    U, V, O = m[:, 0], m[:, 1], m[:, 3]
    if p.boundary == P.BOUNDARY_SPHERE:
        c = np.asarray(p.sph_center, np.float64)
        a = np.clip(np.dot(c - O, U) / np.dot(U, U), -1, 1); b = np.clip(np.dot(c - O, V) / np.dot(V, V), -1, 1)
        q = O + a * U + b * V - c
        return float(np.dot(q, q)) < float(p.sph_radius) ** 2
    lo, hi = np.asarray(p.bmin, np.float64), np.asarray(p.bmax, np.float64)
    c, h = 0.5 * (lo + hi) - O, 0.5 * (hi - lo)
    E = np.eye(3)
    axes = [E[0], E[1], E[2], U, V, np.cross(U, V)] + [np.cross(E[i], w) for i in range(3) for w in (U, V)]
    for L in axes:            # separating axis theorem; touching counts as meeting
        if abs(np.dot(c, L)) > np.dot(h, np.abs(L)) + abs(np.dot(U, L)) + abs(np.dot(V, L)):
            return False
    return True


def _disk_outside(p, m):
    """the disk O + a U + b V, a^2 + b^2 <= 1, lies outside the medium shape: its point closest to the sphere's centre lies outside (exact);
    against the cube its circumscribed square must pass the rectangle / box test (conservative)"""
    if p.boundary != P.BOUNDARY_SPHERE:
        return not _rect_meets_shape(p, m)
    U, V, O = m[:, 0], m[:, 1], m[:, 3]
    d = np.asarray(p.sph_center, np.float64) - O
    a, b = np.dot(d, U) / np.dot(U, U), np.dot(d, V) / np.dot(V, V)
    r = np.hypot(a, b)
    if r > 1:
        a, b = a / r, b / r
    q = a * U + b * V - d
    return not float(np.dot(q, q)) < float(p.sph_radius) ** 2


def _sphere_clear(p, c, R, flipped):
    """the sphere (centre c, radius R) is clear of the medium shape: apart from it, or -- flipped only -- around it"""
    if p.boundary == P.BOUNDARY_SPHERE:
        d = float(np.linalg.norm(c - np.asarray(p.sph_center, np.float64)))
        return d > R + p.sph_radius or (flipped and d + p.sph_radius < R)
    lo, hi = np.asarray(p.bmin, np.float64), np.asarray(p.bmax, np.float64)
    near = np.maximum(np.maximum(lo - c, c - hi), 0.0)
    far = np.maximum(np.abs(c - lo), np.abs(c - hi))
    return float(np.dot(near, near)) > R * R or (flipped and float(np.dot(far, far)) < R * R)


def _point_in_shape(p, x):
    x = np.asarray(x, np.float32)
    if p.boundary == P.BOUNDARY_AABB:
        return bool(np.all(x >= np.asarray(p.bmin, np.float32)) and np.all(x <= np.asarray(p.bmax, np.float32)))
    if p.boundary == P.BOUNDARY_SPHERE:
        return float(np.sum((x - np.asarray(p.sph_center, np.float32)) ** 2)) < float(p.sph_radius) ** 2
    return _sdf_value(p, x) < 0 if p.sdf is not None else False


def validate_emitters(p):
    """The refusals of an emitter list (p.emitters), as mer_render applies them: MerError.  No GPU needed."""
    ems = list(getattr(p, "emitters", None) or [])
    if not ems:
        return
    if len(ems) > P.MAX_EMITTERS:
        raise MerError("emitter list: at most %d entries (MER_MAX_EMITTERS)" % P.MAX_EMITTERS)
    if any(v != 0 for v in p.point_intensity) or any(v != 0 for v in p.area_radiance):
        raise MerError("emitter list: the point_* / area_* emitter fields must be zero when n_emitters > 0")
    has_rect, outside_point, n_env = False, False, 0
    for j, e in enumerate(ems):
        at = "emitter list, entry %d: " % j
        w = float(e.get("sampling_weight", 1.0))
        if not (np.isfinite(w) and w > 0):
            raise MerError(at + "samplingWeight must be positive")
        if e["type"] == P.EMITTER_POINT:
            if not all(v >= 0 for v in e["intensity"]):
                raise MerError(at + "emitter radiance / intensity must be non-negative")
            inside = _point_in_shape(p, e["position"])
            if p.boundary_bsdf == P.BSDF_HROUGHDIELECTRIC and inside:
                raise MerError(at + "hroughdielectric: the point emitter must lie outside the medium shape")
            outside_point = outside_point or (p.boundary != P.BOUNDARY_SDF and not inside)
        elif e["type"] == P.EMITTER_SPOT:
            err = P.spot_error(e.get("to_world"), e["cutoff_deg"], e["beam_deg"])
            if err:
                raise MerError(at + err)
            if not all(np.isfinite(v) and v >= 0 for v in e["intensity"]):
                raise MerError(at + "emitter radiance / intensity must be non-negative")
            inside = _point_in_shape(p, P.spot_position(e))
            if p.boundary_bsdf == P.BSDF_HROUGHDIELECTRIC and inside:
                raise MerError(at + "hroughdielectric: the spot emitter must lie outside the medium shape")
            outside_point = outside_point or (p.boundary != P.BOUNDARY_SDF and not inside)
        elif e["type"] == P.EMITTER_COLLIMATED:
            if getattr(p, "integrator", P.INTEGRATOR_VOLPATH) != P.INTEGRATOR_PTRACER:
                raise MerError(at + "a collimated emitter is a delta in position and direction: no camera path can sample it (it would render black); use integrator = ptracer")
            err = P.collimated_error(e.get("to_world"))
            if err:
                raise MerError(at + err)
            if not all(np.isfinite(v) and v >= 0 for v in e["power"]):
                raise MerError(at + "emitter radiance / intensity must be non-negative")
        elif e["type"] in P.AREA_TYPES:
            if p.rif_mode != P.RIF_CONST:
                raise MerError(at + "the area emitter is built for straight rays (rif_mode = CONST)")
            if p.boundary_bsdf != P.BSDF_NULL or p.boundary == P.BOUNDARY_SDF:
                raise MerError(at + "the area emitter needs an index-matched cube / sphere boundary")
            if not all(v >= 0 for v in e["radiance"]):
                raise MerError(at + "emitter radiance / intensity must be non-negative")
            if e["type"] != P.EMITTER_AREA:
                err = P.area_shape_error(e["type"], e.get("to_world"))
                if err:
                    raise MerError(at + err)
            m = np.array(_rows3x4(e.get("to_world")), np.float64).reshape(3, 4)
            if e["type"] == P.EMITTER_AREA_SPHERE:
                if not _sphere_clear(p, m[:, 3], float(np.float32(np.linalg.norm(m[:, 0]))), np.linalg.det(m[:, :3]) < 0):
                    raise MerError(at + "the area emitter's sphere must be clear of the medium shape (apart from it, or with inward normals around it)")
            elif e["type"] == P.EMITTER_AREA_DISK:
                if not _disk_outside(p, m):
                    raise MerError(at + "the area emitter's disk must lie outside the medium shape")
            elif _rect_meets_shape(p, m):
                raise MerError(at + "the area emitter's rectangle must lie outside the medium shape")
            has_rect = True
        elif e["type"] == P.EMITTER_ENVMAP:
            if n_env or any(v != 0 for v in p.env_radiance):
                raise MerError(at + "The scene may only contain one environment emitter (an envmap entry excludes a second one and a non-zero env_radiance)")
            n_env += 1
            err = P.envmap_error(e["image"], e.get("to_world"), e.get("scale", 1.0), w) if e.get("image") is not None else None
            if err:
                raise MerError(at + err)
        else:
            raise MerError(at + "unknown emitter type")
    if has_rect and outside_point:
        raise MerError("emitter list: a point or spot emitter outside the medium shape cannot be combined with an area emitter")


def _is_rotation(m, tol=1e-4):
    R = np.asarray(m, np.float64)[:3, :3].astype(np.float32).astype(np.float64)
    return bool(np.all(np.isfinite(R)) and np.max(np.abs(R @ R.T - np.eye(3))) <= tol and np.linalg.det(R) > 0)


def validate_integrator(p):
    """The refusals of the integrator field, and of a scene outside the light tracer's scope (integrator = ptracer), as mer_render
    applies them before anything reaches the device: MerError.  No GPU needed."""
    integ = getattr(p, "integrator", P.INTEGRATOR_VOLPATH)
    if integ not in (P.INTEGRATOR_VOLPATH, P.INTEGRATOR_PTRACER):
        raise MerError("integrator: unknown integrator (volpath, ptracer)")
    if integ != P.INTEGRATOR_PTRACER:
        return
    at = "ptracer: "
    if p.sensor != P.SENSOR_PERSPECTIVE:
        raise MerError(at + "light paths are connected to the perspective sensor only (orthographic, thinlens and telecentric are not built)")
    if not _is_rotation(p.cam_to_world):
        raise MerError(at + "cam_to_world must be a rigid transformation (its inverse is taken as the transpose)")
    if any(v != 0 for v in p.env_radiance):
        raise MerError(at + "a constant environment (env_radiance) is not built for light tracing")
    if any(v != 0 for v in p.emission):
        raise MerError(at + "medium emission is not built for light tracing")
    if any(v != 0 for v in p.point_intensity) or any(v != 0 for v in p.area_radiance):
        raise MerError(at + "emitters are given as list entries (mer_scene_desc.emitters); the point_* / area_* fields must be zero")
    ems = list(getattr(p, "emitters", None) or [])
    if not ems:
        raise MerError(at + "the scene has no emitter (list entries of kind point, spot or collimated)")
    for j, e in enumerate(ems[:P.MAX_EMITTERS]):
        ej = at + "emitter list, entry %d: " % j
        if e["type"] == P.EMITTER_ENVMAP:
            raise MerError(ej + "an envmap emitter is not built for light tracing")
        if e["type"] in P.AREA_TYPES:
            raise MerError(ej + "area emitters are not built for light tracing")
        if e["type"] == P.EMITTER_SPOT and not _is_rotation(np.array(_rows3x4(e.get("to_world"))).reshape(3, 4)):
            raise MerError(ej + "a spot emitter's 'toWorld' must be free of scale for light tracing (its cone is sampled about the z axis)")
    if p.boundary == P.BOUNDARY_SDF:
        raise MerError(at + "the signed-distance boundary is not built for light tracing (cube or sphere)")
    if p.boundary_bsdf != P.BSDF_NULL:
        raise MerError(at + "dielectric boundaries are not built for light tracing (the index-matched null boundary)")
    if p.sigma_mode == P.SIGMA_GRID and p.method == P.METHOD_SIMPSON:
        raise MerError(at + "method = simpson is not built for light tracing (woodcock)")


def _upload_scene_envmap(ctx, p, vols):
    """upload_scene: the image of the emitter list's envmap entry (validated first), appended to vols; None without one"""
    ems = [e for e in (getattr(p, "emitters", None) or []) if e["type"] == P.EMITTER_ENVMAP and e.get("image") is not None]
    if not ems:
        return None
    validate_emitters(p)
    env = ctx.upload_envmap(ems[0]["image"])
    vols.append(env)
    return env


class Shard(C.Structure):
    _fields_ = [("spp_begin", C.c_int32), ("spp_count", C.c_int32), ("spp_stride", C.c_int32),
                ("tile_rank", C.c_int32), ("tile_count", C.c_int32)]


class MerError(RuntimeError):
    """Mirrors the reference's Log(EError) -> std::runtime_error (src/libcore/logger.cpp:100-147)."""


class FluenceDesc(C.Structure):
    """mer_fluence_desc: res cells per axis (x, y, z) over the box bmin ... bmax"""
    _fields_ = [("res", C.c_int32 * 3), ("bmin", C.c_float * 3), ("bmax", C.c_float * 3)]


FLUENCE_TOTALS = ("paths", "escaped", "dropped", "ended")        # mer_fluence_read's totals: [0], [1..3], [4..6], [7]


def fluence_desc(res, bmin, bmax):
    d = FluenceDesc()
    d.res[:] = [int(v) for v in res]
    d.bmin[:] = [float(v) for v in bmin]
    d.bmax[:] = [float(v) for v in bmax]
    return d


def _validate_box(desc, at):
    """the box checks every voxel grid shares (res, bmin, bmax of desc), under the entry point's prefix"""
    cells = 1
    for a in range(3):
        if desc.res[a] < 1 or desc.res[a] > 1024:
            raise MerError(at + "res must lie in 1 ... 1024 on every axis")
        if not (np.isfinite(desc.bmin[a]) and np.isfinite(desc.bmax[a])):
            raise MerError(at + "bmin / bmax must be finite")
        if not desc.bmin[a] < desc.bmax[a]:
            raise MerError(at + "bmin must be below bmax on every axis")
        cells *= desc.res[a]
    if cells > 1 << 27:
        raise MerError(at + "more than 2^27 cells")


def _validate_raster(t, at, res_what, frames):
    """the raster / gate / cone checks an exitance map and a detector (one frame) share, under the entry point's prefix"""
    if t.boundary not in (P.BOUNDARY_AABB, P.BOUNDARY_SPHERE):
        raise MerError(at + "boundary must be the cube (MER_BOUNDARY_AABB) or the sphere (MER_BOUNDARY_SPHERE)")
    for a in range(2):
        if t.res[a] < 1 or t.res[a] > 4096:
            raise MerError(at + res_what + " must lie in 1 ... 4096 on both axes")
    if frames < 1 or frames > 4096:
        raise MerError(at + "frames must lie in 1 ... 4096")
    if not np.isfinite(t.t_bin) or t.t_bin < 0:
        raise MerError(at + "t_bin must be finite and at least 0")
    if t.t_bin == 0 and frames != 1:
        raise MerError(at + "a steady map (t_bin == 0) has one frame")
    if not np.isfinite(t.t_min):
        raise MerError(at + "t_min must be finite")
    if not (t.cos_min >= 0 and t.cos_min < 1):
        raise MerError(at + "cos_min must lie in 0 <= cos_min < 1")
    if t.reserved != 0:
        raise MerError(at + "reserved must be 0")


def validate_fluence(desc):
    """The refusals of mer_fluence_create, with its messages: MerError.  No GPU needed."""
    _validate_box(desc, "mer_fluence_create: ")


def validate_fluence_track(desc):
    """The refusals of mer_fluence_track_create: the same checks under its own prefix"""
    _validate_box(desc, "mer_fluence_track_create: ")


class FluenceTimeDesc(C.Structure):
    """mer_fluence_time_desc: the box of a FluenceDesc and `frames` bins of width t_bin from t_min on in optical path length"""
    _fields_ = [("res", C.c_int32 * 3), ("bmin", C.c_float * 3), ("bmax", C.c_float * 3),
                ("frames", C.c_int32), ("t_min", C.c_float), ("t_bin", C.c_float), ("reserved", C.c_int32)]


def fluence_time_desc(res, bmin, bmax, frames, t_min, t_bin):
    d = FluenceTimeDesc()
    d.res[:] = [int(v) for v in res]
    d.bmin[:] = [float(v) for v in bmin]
    d.bmax[:] = [float(v) for v in bmax]
    d.frames, d.t_min, d.t_bin, d.reserved = int(frames), float(t_min), float(t_bin), 0
    return d


def validate_fluence_time(desc):
    """The refusals of mer_fluence_time_create, with its messages: MerError.  No GPU needed."""
    at = "mer_fluence_time_create: "
    _validate_box(desc, at)
    if desc.frames < 1 or desc.frames > 4096:
        raise MerError(at + "frames must lie in 1 ... 4096")
    if not np.isfinite(desc.t_min):
        raise MerError(at + "t_min must be finite")
    if not (np.isfinite(desc.t_bin) and desc.t_bin > 0):
        raise MerError(at + "t_bin must be finite and greater than 0")
    if desc.reserved != 0:
        raise MerError(at + "reserved must be 0")
    if desc.res[0] * desc.res[1] * desc.res[2] * desc.frames > 1 << 27:
        raise MerError(at + "more than 2^27 cells x frames")


class ExitanceDesc(C.Structure):
    """mer_exitance_desc: res = (res_u, res_v) cells on every face of the medium shape's boundary (6 faces for the cube, 1 for the sphere),
    `frames` bins of width t_bin from t_min on in optical path length (a steady map: frames 1, t_bin 0) and the acceptance cone cos_min"""
    _fields_ = [("boundary", C.c_int32), ("res", C.c_int32 * 2), ("frames", C.c_int32), ("t_min", C.c_float), ("t_bin", C.c_float),
                ("cos_min", C.c_float), ("reserved", C.c_int32)]


EXITANCE_TOTALS = ("paths", "escaped", "missed", "ended", "late", "rejected", "binned")     # mer_exitance_read's totals: [0], [1..3], [4..6], [7], [8..10], [11..13], [14]


def exitance_desc(boundary, res, frames=1, t_min=0.0, t_bin=0.0, cos_min=0.0):
    d = ExitanceDesc()
    d.boundary = int(boundary)
    d.res[:] = [int(v) for v in res]
    d.frames, d.t_min, d.t_bin, d.cos_min, d.reserved = int(frames), float(t_min), float(t_bin), float(cos_min), 0
    return d


def exitance_faces(boundary):
    return 1 if boundary == P.BOUNDARY_SPHERE else 6


def validate_exitance(desc):
    """The refusals of mer_exitance_create, with its messages: MerError.  No GPU needed."""
    at = "mer_exitance_create: "
    _validate_raster(desc, at, "res", desc.frames)
    if desc.frames * exitance_faces(desc.boundary) * desc.res[0] * desc.res[1] > 1 << 27:
        raise MerError(at + "more than 2^27 cells x faces x frames")


MAX_FREQUENCIES = 8           # MER_MAX_FREQUENCIES


class FluenceFDDesc(C.Structure):
    """mer_fluence_fd_desc: the box of a FluenceDesc and n_freq wavenumbers k >= 0 in radians per unit of optical path length (k = 2 pi f / c0;
    0: the steady state).  No implicit padding: wavenumber starts at byte 48"""
    _fields_ = [("res", C.c_int32 * 3), ("bmin", C.c_float * 3), ("bmax", C.c_float * 3), ("n_freq", C.c_int32), ("reserved", C.c_int32 * 2),
                ("wavenumber", C.c_double * MAX_FREQUENCIES)]


class ExitanceFDDesc(C.Structure):
    """mer_exitance_fd_desc: the raster and cone of an ExitanceDesc and n_freq wavenumbers; wavenumber starts at byte 24"""
    _fields_ = [("boundary", C.c_int32), ("res", C.c_int32 * 2), ("cos_min", C.c_float), ("n_freq", C.c_int32), ("reserved", C.c_int32),
                ("wavenumber", C.c_double * MAX_FREQUENCIES)]


def _set_wavenumbers(d, wavenumbers):
    """n_freq and the wavenumber array of a frequency-domain desc; a list no desc can hold is refused here, under the name of n_freq's check"""
    k = [float(v) for v in np.atleast_1d(np.asarray(wavenumbers, np.float64))]
    d.n_freq = len(k)
    d.wavenumber[:] = (k + [0.0] * MAX_FREQUENCIES)[:MAX_FREQUENCIES]
    return d


def fluence_fd_desc(res, bmin, bmax, wavenumbers):
    d = FluenceFDDesc()
    d.res[:] = [int(v) for v in res]
    d.bmin[:] = [float(v) for v in bmin]
    d.bmax[:] = [float(v) for v in bmax]
    return _set_wavenumbers(d, wavenumbers)


def exitance_fd_desc(boundary, res, wavenumbers, cos_min=0.0):
    d = ExitanceFDDesc()
    d.boundary = int(boundary)
    d.res[:] = [int(v) for v in res]
    d.cos_min = float(cos_min)
    return _set_wavenumbers(d, wavenumbers)


def _validate_frequencies(desc, at, reserved):
    """the wavenumber checks the two frequency-domain recorders share, under the entry point's prefix"""
    if desc.n_freq < 1 or desc.n_freq > MAX_FREQUENCIES:
        raise MerError(at + "n_freq must lie in 1 ... 8")
    for j in range(desc.n_freq):
        if not np.isfinite(desc.wavenumber[j]) or desc.wavenumber[j] < 0:
            raise MerError(at + "a wavenumber must be finite and at least 0")
    for j in range(desc.n_freq, MAX_FREQUENCIES):
        if not desc.wavenumber[j] == 0:
            raise MerError(at + "the entries of wavenumber past n_freq must be 0")
    if any(v != 0 for v in reserved):
        raise MerError(at + "reserved must be 0")


def validate_fluence_fd(desc):
    """The refusals of mer_fluence_fd_create, with its messages: MerError.  No GPU needed."""
    at = "mer_fluence_fd_create: "
    _validate_box(desc, at)
    _validate_frequencies(desc, at, desc.reserved[:])
    if desc.res[0] * desc.res[1] * desc.res[2] * 2 * desc.n_freq > 1 << 27:
        raise MerError(at + "more than 2^27 cells x 2 x n_freq")


def validate_exitance_fd(desc):
    """The refusals of mer_exitance_fd_create, with its messages: MerError.  No GPU needed."""
    at = "mer_exitance_fd_create: "
    _validate_raster(SimpleNamespace(boundary=desc.boundary, res=desc.res, t_bin=0.0, t_min=0.0, cos_min=desc.cos_min, reserved=0), at, "res", 1)
    _validate_frequencies(desc, at, [desc.reserved])
    if 2 * desc.n_freq * exitance_faces(desc.boundary) * desc.res[0] * desc.res[1] > 1 << 27:
        raise MerError(at + "more than 2^27 cells x faces x 2 x n_freq")


class DetectorDesc(C.Structure):
    """mer_detector_desc: the raster of an exitance map (res = (res_u, res_v) cells per face), one face of it, the half-open cell window
    iu0 <= iu < iu1, iv0 <= iv < iv1 on that face, the acceptance cone cos_min and the gate (t_min, t_bin) in optical path length (t_bin 0: none)"""
    _fields_ = [("boundary", C.c_int32), ("res", C.c_int32 * 2), ("face", C.c_int32), ("iu0", C.c_int32), ("iu1", C.c_int32),
                ("iv0", C.c_int32), ("iv1", C.c_int32), ("cos_min", C.c_float), ("t_min", C.c_float), ("t_bin", C.c_float), ("reserved", C.c_int32)]


class SensitivityDesc(C.Structure):
    """mer_sensitivity_desc: the box of a FluenceDesc and the detector"""
    _fields_ = [("res", C.c_int32 * 3), ("bmin", C.c_float * 3), ("bmax", C.c_float * 3), ("det", DetectorDesc)]


# mer_sensitivity_read's totals: [0], [1..3], [4..6], [7], [8], [9..11], [12]
SENSITIVITY_TOTALS = ("paths", "detected_weight", "dropped", "ended", "detected", "weight_length", "disagreements")


def detector_desc(boundary, res, face, window=None, cos_min=0.0, t_min=0.0, t_bin=0.0):
    """window = (iu0, iu1, iv0, iv1); None: the whole face"""
    d = DetectorDesc()
    d.boundary, d.face = int(boundary), int(face)
    d.res[:] = [int(v) for v in res]
    d.iu0, d.iu1, d.iv0, d.iv1 = [int(v) for v in (window if window is not None else (0, d.res[0], 0, d.res[1]))]
    d.cos_min, d.t_min, d.t_bin, d.reserved = float(cos_min), float(t_min), float(t_bin), 0
    return d


def sensitivity_desc(res, bmin, bmax, detector):
    d = SensitivityDesc()
    d.res[:] = [int(v) for v in res]
    d.bmin[:] = [float(v) for v in bmin]
    d.bmax[:] = [float(v) for v in bmax]
    C.memmove(C.byref(d.det), C.byref(detector), C.sizeof(DetectorDesc))
    return d


def validate_sensitivity(desc):
    """The refusals of mer_sensitivity_create, with its messages: MerError.  No GPU needed."""
    _validate_sensitivity(desc, "mer_sensitivity_create: ")


def _validate_sensitivity(desc, at):
    _validate_box(desc, at)
    t = desc.det
    _validate_raster(t, at, "detector res", 1)
    if t.face < 0 or t.face >= exitance_faces(t.boundary):
        raise MerError(at + "face must be one of the boundary's faces (0 ... 5 for the cube, 0 for the sphere)")
    if t.iu0 < 0 or t.iu1 > t.res[0] or t.iv0 < 0 or t.iv1 > t.res[1]:
        raise MerError(at + "the window must lie inside the raster (0 <= iu0, iu1 <= res[0], 0 <= iv0, iv1 <= res[1])")
    if not (t.iu0 < t.iu1 and t.iv0 < t.iv1):
        raise MerError(at + "the window is empty (iu0 < iu1 and iv0 < iv1 are required)")


class SensitivityArrayDesc(C.Structure):
    """mer_sensitivity_array_desc: the box and the detector of a SensitivityDesc; one detector is bin_u x bin_v raster cells of the window,
    gate g the exits with floorf((l - t_min) / t_bin) == g for 0 <= g < gates; scatter = 1 also records the scattering grids K"""
    _fields_ = [("res", C.c_int32 * 3), ("bmin", C.c_float * 3), ("bmax", C.c_float * 3), ("det", DetectorDesc),
                ("bin_u", C.c_int32), ("bin_v", C.c_int32), ("gates", C.c_int32), ("scatter", C.c_int32), ("reserved", C.c_int32 * 2)]


# mer_sensitivity_read_array's totals: SENSITIVITY_TOTALS, then [13..15]; its meas[m]: [0..2], [3], [4..6], [7]
SENSITIVITY_ARRAY_TOTALS = SENSITIVITY_TOTALS + ("collisions_dropped",)
SENSITIVITY_MEAS = ("detected_weight", "detected", "weight_collisions")


def sensitivity_array_desc(res, bmin, bmax, detector, bins, gates=1, scatter=False):
    """bins = (bin_u, bin_v); None: one detector, the whole window"""
    d = SensitivityArrayDesc()
    d.res[:] = [int(v) for v in res]
    d.bmin[:] = [float(v) for v in bmin]
    d.bmax[:] = [float(v) for v in bmax]
    C.memmove(C.byref(d.det), C.byref(detector), C.sizeof(DetectorDesc))
    d.bin_u, d.bin_v = [int(v) for v in (bins if bins is not None else (d.det.iu1 - d.det.iu0, d.det.iv1 - d.det.iv0))]
    d.gates, d.scatter = int(gates), int(scatter)
    d.reserved[:] = [0, 0]
    return d


def sensitivity_array_shape(d):
    """(1 + scatter, gates, ndv, ndu) of a valid SensitivityArrayDesc"""
    return (1 + d.scatter, d.gates, (d.det.iv1 - d.det.iv0) // d.bin_v, (d.det.iu1 - d.det.iu0) // d.bin_u)


def validate_sensitivity_array(desc):
    """The refusals of mer_sensitivity_array_create, with its messages: MerError.  No GPU needed."""
    at = "mer_sensitivity_array_create: "
    _validate_sensitivity(desc, at)
    t = desc.det
    if desc.bin_u < 1 or desc.bin_v < 1:
        raise MerError(at + "bin_u and bin_v must be at least 1")
    if (t.iu1 - t.iu0) % desc.bin_u or (t.iv1 - t.iv0) % desc.bin_v:
        raise MerError(at + "bin_u and bin_v must divide the window (iu1 - iu0 and iv1 - iv0)")
    if desc.gates < 1:
        raise MerError(at + "gates must be at least 1")
    if desc.gates > 1 and t.t_bin == 0:
        raise MerError(at + "several gates need t_bin > 0")
    if desc.scatter not in (0, 1):
        raise MerError(at + "scatter must be 0 or 1")
    if desc.reserved[0] != 0 or desc.reserved[1] != 0:
        raise MerError(at + "reserved must be 0")
    if int(np.prod(sensitivity_array_shape(desc), dtype=np.int64)) * desc.res[0] * desc.res[1] * desc.res[2] > 1 << 27:
        raise MerError(at + "more than 2^27 cells x measurements x (1 + scatter)")


def _box_shape(d):
    return (d.res[2], d.res[1], d.res[0])


# The kinds of recorder a context hands out (Context._recorder_*): the family whose clear / destroy / render entry points take the handle
# (mer_<family>_clear, mer_<family>_destroy, mer_render_<family>), the C create function, the desc builder, the validator, the read entry point
# with its totals count, the shape of the sums (without the 3 channels) from the desc and what the family's other reads call this kind: they
# refuse it with "<their name>: <what>: use <read>".  A new kind is one row here and the public methods that name it.
_Recorder = collections.namedtuple("_Recorder", "family create desc validate read totals shape what")
_RECORDERS = {
    "fluence": _Recorder("fluence", "mer_fluence_create", fluence_desc, validate_fluence, "mer_fluence_read", 8, _box_shape, "steady-state grid"),
    "fluence_track": _Recorder("fluence", "mer_fluence_track_create", fluence_desc, validate_fluence_track, "mer_fluence_read", 8, _box_shape,
                               "steady-state grid"),
    "fluence_time": _Recorder("fluence", "mer_fluence_time_create", fluence_time_desc, validate_fluence_time, "mer_fluence_time_read", 12,
                              lambda d: (d.frames,) + _box_shape(d), "time-resolved grid"),
    "fluence_fd": _Recorder("fluence", "mer_fluence_fd_create", fluence_fd_desc, validate_fluence_fd, "mer_fluence_fd_read", 8,
                            lambda d: (d.n_freq, 2) + _box_shape(d), "frequency-domain grid"),
    "exitance": _Recorder("exitance", "mer_exitance_create", exitance_desc, validate_exitance, "mer_exitance_read", 16,
                          lambda d: (d.frames, exitance_faces(d.boundary), d.res[1], d.res[0]), "steady or time-gated map"),
    "exitance_fd": _Recorder("exitance", "mer_exitance_fd_create", exitance_fd_desc, validate_exitance_fd, "mer_exitance_fd_read", 16,
                             lambda d: (d.n_freq, 2, exitance_faces(d.boundary), d.res[1], d.res[0]), "frequency-domain map"),
    "sensitivity": _Recorder("sensitivity", "mer_sensitivity_create", sensitivity_desc, validate_sensitivity, "mer_sensitivity_read", 16, _box_shape, None),
    # read through Context.sensitivity_read_array (which takes the handles of both rows) and, with one measurement and no K, Context.sensitivity_read
    "sensitivity_array": _Recorder("sensitivity", "mer_sensitivity_array_create", sensitivity_array_desc, validate_sensitivity_array, "mer_sensitivity_read_array", 16,
                                   lambda d: sensitivity_array_shape(d) + _box_shape(d), None),
}


def lib(path=None):
    """The C-ABI library (ctypes).  path = None: libmer.so; Context(check=True) loads libmer_check.so beside it."""
    path = path or LIB_PATH
    if path not in _LIBS:
        if not os.path.exists(path):
            raise MerError("%s is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "-- there is no CPU fallback for the hot path" % (os.path.basename(path), path))
        L = C.CDLL(path)
        L.mer_last_error.restype = C.c_char_p
        L.mer_last_error.argtypes = [C.c_void_p]
        for s in SYMBOLS:
            if s not in ("mer_last_error", "mer_context_destroy", "mer_multi_destroy", "mer_multi_last_error", "mer_multi_context"):
                getattr(L, s).restype = C.c_int
        L.mer_context_destroy.restype = None
        L.mer_multi_destroy.restype = None
        L.mer_multi_destroy.argtypes = [C.c_void_p]
        L.mer_multi_last_error.restype = C.c_char_p
        L.mer_multi_last_error.argtypes = [C.c_void_p]
        L.mer_multi_context.restype = C.c_void_p
        L.mer_multi_context.argtypes = [C.c_void_p, C.c_int32]
        _LIBS[path] = L
    return _LIBS[path]


def _fp(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


class Volume:
    def __init__(self, ctx, handle, desc, layout):
        self.ctx, self.handle, self.desc, self.layout = ctx, handle, desc, layout
        self.has_spline = False

    def build_spline(self):
        self.ctx._check(self.ctx.lib.mer_volume_build_spline(self.ctx.h, C.c_int32(self.handle)))
        self.has_spline = True
        return self

    def download_spline(self):
        out = np.empty((self.desc.res[2], self.desc.res[1], self.desc.res[0]), np.float32)
        self.ctx._check(self.ctx.lib.mer_volume_download_spline(self.ctx.h, C.c_int32(self.handle), _fp(out)))
        return out

    def destroy(self):
        if self.handle:
            if isinstance(self.ctx, MultiContext):
                self.ctx.destroy_volume(self)
            else:
                self.ctx.lib.mer_volume_destroy(self.ctx.h, C.c_int32(self.handle))
            self.handle = 0


class Context:
    """One context per (process, GPU)."""

    def __init__(self, device_id=0, check=False, _borrowed=None, **options):
        """check=True: the bounds-checking build of the library (libmer_check.so); options: mer_context_set_option names."""
        self.lib = lib(CHECK_LIB_PATH if check else None)
        self.owned = _borrowed is None
        if _borrowed is not None:                      # a context owned by a MultiContext
            self.h = C.c_void_p(_borrowed)
        else:
            self.h = C.c_void_p()
            rc = self.lib.mer_context_create(C.c_int32(device_id), C.byref(self.h))
            if rc != 0:
                raise MerError(self.lib.mer_last_error(None).decode())
        self.device_id = device_id
        self._recorders = {}                           # handle -> (kind in _RECORDERS, shape of its sums) of the live grids and maps
        for k, v in options.items():
            self.set_option(k, v)

    def _check(self, rc):
        if rc != 0:
            raise MerError(self.lib.mer_last_error(self.h).decode())

    def close(self):
        if self.h and self.owned:
            self.lib.mer_context_destroy(self.h)
        self.h = C.c_void_p()

    def set_option(self, name, value):
        self._check(self.lib.mer_context_set_option(self.h, name.encode(), C.c_int64(int(value))))

    def get_option(self, name):
        v = C.c_int64()
        self._check(self.lib.mer_context_get_option(self.h, name.encode(), C.byref(v)))
        return v.value

    def options(self, **kw):
        """context manager: set options for the duration of a `with` block, then restore them"""
        ctx = self

        class _Scope:
            def __enter__(self_):
                self_.old = {k: ctx.get_option(k) for k in kw}
                for k, v in kw.items():
                    ctx.set_option(k, v)
                return ctx

            def __exit__(self_, *a):
                for k, v in self_.old.items():
                    ctx.set_option(k, v)
        return _Scope()

    def debug_bounds(self):
        """-> (enabled, violations, kind, index, limit) of the bounds-checking build; resets the record"""
        en = C.c_int32(); out = (C.c_uint64 * 4)()
        self._check(self.lib.mer_debug_bounds(self.h, C.byref(en), out))
        return bool(en.value), int(out[0]), int(out[1]), int(out[2]), int(out[3])

    def set_stream(self, stream_ptr):
        self._check(self.lib.mer_context_set_stream(self.h, C.c_void_p(stream_ptr)))

    def device_info(self):
        name = C.create_string_buffer(256)
        cu = C.c_int32(); hbm = C.c_int64()
        self._check(self.lib.mer_device_info(self.h, name, C.c_int32(256), C.byref(cu), C.byref(hbm)))
        return name.value.decode(), cu.value, hbm.value

    # ---- volumes -------------------------------------------------------------------------------
    @staticmethod
    def _desc(shape, channels, dtype, aabb_min, aabb_max, to_world=None):
        d = GridDesc()
        d.world_to_volume[:] = [float(v) for v in P.world_to_volume(to_world).reshape(-1)]
        d.res[:] = [shape[2], shape[1], shape[0]]
        d.channels = channels
        d.dtype = dtype
        d.aabb_min[:] = [float(v) for v in aabb_min]
        d.aabb_max[:] = [float(v) for v in aabb_max]
        return d

    def upload_volume(self, data, aabb_min, aabb_max, layout=LAYOUT_DENSE, to_world=None):
        """data[z][y][x](,c): float32 or uint8 numpy array; to_world: the volume plugin's `toWorld` (3x4 or 4x4), None = identity."""
        a = np.ascontiguousarray(data)
        if a.dtype != np.uint8:
            a = a.astype(np.float32, copy=False)
        ch = 1 if a.ndim == 3 else a.shape[3]
        d = self._desc(a.shape, ch, P.VOL_U8 if a.dtype == np.uint8 else P.VOL_F32, aabb_min, aabb_max, to_world)
        h = C.c_int32()
        self._check(self.lib.mer_volume_upload(self.h, C.byref(d), _fp(a), C.c_int32(layout), C.byref(h)))
        return Volume(self, h.value, d, layout)

    def upload_volume_dev(self, dev_ptr, shape, aabb_min, aabb_max, layout=LAYOUT_DENSE):
        d = self._desc(shape, 1, P.VOL_F32, aabb_min, aabb_max)
        h = C.c_int32()
        self._check(self.lib.mer_volume_upload_dev(self.h, C.byref(d), C.c_void_p(dev_ptr), C.c_int32(layout), C.byref(h)))
        return Volume(self, h.value, d, layout)

    def sdf_from_mesh(self, vertices, triangles, res, aabb_min, aabb_max, layout=LAYOUT_DENSE, max_triangles_per_launch=0, return_winding=False):
        """mer_sdf_from_mesh: the signed-distance grid (negative inside) of a triangle mesh as a Volume.  vertices float [V][3], triangles
        int [T][3], res = (nx, ny, nz); max_triangles_per_launch = 0: the library's default chunk.  return_winding: -> (Volume, w[z][y][x])."""
        v = np.ascontiguousarray(np.asarray(vertices, np.float32).reshape(-1, 3))
        t = np.ascontiguousarray(np.asarray(triangles, np.int32).reshape(-1, 3))
        nx, ny, nz = (int(r) for r in res)
        d = self._desc((nz, ny, nx), 1, P.VOL_F32, aabb_min, aabb_max)
        w = np.empty((nz, ny, nx), np.float32) if return_winding else None
        h = C.c_int32()
        self._check(self.lib.mer_sdf_from_mesh(self.h, C.byref(d), _fp(v), C.c_int64(v.shape[0]), _fp(t), C.c_int64(t.shape[0]),
                                               C.c_int32(max_triangles_per_launch), C.c_int32(layout), _fp(w) if w is not None else None, C.byref(h)))
        vol = Volume(self, h.value, d, layout)
        return (vol, w) if return_winding else vol

    def volume_download(self, vol):
        """mer_volume_download: the dense float32 payload [z][y][x] of a 1-channel float32 Volume"""
        if vol.desc is None:
            raise MerError("volume_download: an envmap handle has no grid payload")
        if vol.desc.channels != 1 or vol.desc.dtype != P.VOL_F32:
            raise MerError("volume_download: only a 1-channel float32 volume can be downloaded")
        out = np.empty((vol.desc.res[2], vol.desc.res[1], vol.desc.res[0]), np.float32)
        self._check(self.lib.mer_volume_download(self.h, C.c_int32(vol.handle), _fp(out)))
        return out

    def synth_volume(self, kind, N, layout=LAYOUT_DENSE, aabb_min=(-1, -1, -1), aabb_max=(1, 1, 1)):
        """Synthetic field generated in HBM (0 = sigma_t density, 1 = linear RIF, 2 = radial RIF)."""
        ptr = C.c_void_p()
        self._check(self.lib.mer_synth_field_dev(self.h, C.c_int32(kind), C.c_int32(N), C.byref(ptr)))
        try:
            v = self.upload_volume_dev(ptr.value, (N, N, N), aabb_min, aabb_max, layout)
        finally:
            self.lib.mer_device_free(self.h, ptr)
        return v

    # ---- scene ---------------------------------------------------------------------------------
    def scene_desc(self, p, density=None, albedo_grid=None, rif=None, sdf=None, envmap=None):
        """p: params.SceneParams; volumes as Volume objects; envmap: the Volume of upload_envmap for the list's envmap entry (or the entry's
        "handle")."""
        s = SceneDesc()
        s.width, s.height = p.width, p.height
        s.fov_x_deg, s.near_clip, s.far_clip = p.fov_x_deg, p.near_clip, p.far_clip
        s.cam_to_world[:] = [float(v) for v in np.asarray(p.cam_to_world, np.float32).reshape(-1)]
        s.rfilter, s.rfilter_param = p.rfilter, p.rfilter_param
        validate_sensor(p)
        validate_integrator(p)
        s.integrator = int(getattr(p, "integrator", P.INTEGRATOR_VOLPATH)); s.integrator_reserved = 0
        s.sensor = int(p.sensor); s.sensor_reserved = 0
        lens = p.sensor in (P.SENSOR_THINLENS, P.SENSOR_TELECENTRIC)
        s.aperture_radius = float(p.aperture_radius) if lens else 0.0
        s.focus_distance = float(p.focus_distance) if lens else 0.0
        s.max_depth, s.rr_depth, s.hide_emitters = p.max_depth, p.rr_depth, int(p.hide_emitters)
        s.boundary = p.boundary
        s.bmin[:] = p.bmin; s.bmax[:] = p.bmax
        s.sph_center[:] = p.sph_center; s.sph_radius = p.sph_radius
        s.sigma_mode = p.sigma_mode
        s.sigma_a[:] = p.sigma_a; s.sigma_s[:] = p.sigma_s
        s.strategy, s.channel, s.sampling_density = p.strategy, p.channel, p.sampling_density
        s.medium_sampling_weight = p.medium_sampling_weight
        s.density = density.handle if density is not None else 0
        s.density_scale = p.density_scale
        s.albedo_mode = p.albedo_mode
        s.albedo[:] = p.albedo
        s.albedo_grid = albedo_grid.handle if albedo_grid is not None else 0
        s.rif_mode, s.rif_const = p.rif_mode, p.rif_const
        s.rif = rif.handle if rif is not None else 0
        s.ac_n_o, s.ac_n_max, s.ac_k_r, s.ac_mode = float(p.ac_n_o), float(p.ac_n_max), float(p.ac_k_r), int(p.ac_mode)
        s.method = int(p.method); s.het_stepsize = float(p.het_stepsize)
        s.stepper, s.stepsize = p.stepper, p.stepsize
        s.phase, s.g = p.phase, p.g
        s.tr_estimator = p.tr_estimator
        s.env_radiance[:] = p.env_radiance
        s.emission[:] = p.emission
        s.point_position[:] = p.point_position; s.point_intensity[:] = p.point_intensity
        s.decomposition = p.decomposition; s.min_bound = p.min_bound; s.max_bound = p.max_bound; s.bin_width = p.bin_width
        s.calibrated_transient = int(p.calibrated_transient)
        s.modulation = p.modulation; s.mod_lambda = p.mod_lambda; s.mod_phase_deg = p.mod_phase_deg; s.mod_P = p.mod_P; s.mod_neighbors = p.mod_neighbors
        s.boundary_bsdf = p.boundary_bsdf
        s.sdf = sdf.handle if sdf is not None else 0
        s.aggressive_tracing = int(p.aggressive_tracing); s.sdf_max_error = P.sdf_max_error(p)
        s.area_to_world[:] = _rows3x4(p.area_to_world)
        s.area_radiance[:] = p.area_radiance
        ems = list(getattr(p, "emitters", None) or [])
        validate_emitters(p)
        if ems:
            arr = (EmitterDesc * len(ems))()
            for e, d in zip(arr, ems):
                e.type = int(d["type"]); e.sampling_weight = float(d.get("sampling_weight", 1.0))
                if e.type == P.EMITTER_POINT:
                    e.position[:] = [float(v) for v in d["position"]]; e.intensity[:] = [float(v) for v in d["intensity"]]
                elif e.type == P.EMITTER_SPOT:
                    e.to_world[:] = _rows3x4(d.get("to_world")); e.intensity[:] = [float(v) for v in d["intensity"]]
                    e.cutoff_angle_deg = float(d["cutoff_deg"]); e.beam_width_deg = float(d["beam_deg"])
                elif e.type == P.EMITTER_COLLIMATED:
                    e.to_world[:] = _rows3x4(d.get("to_world")); e.intensity[:] = [float(v) for v in d["power"]]
                elif e.type == P.EMITTER_ENVMAP:
                    e.to_world[:] = _rows3x4(d.get("to_world")); e.env_scale = float(d.get("scale", 1.0)); e.env_reserved = 0.0
                    e.envmap = envmap.handle if envmap is not None else int(d.get("handle", 0))
                else:
                    e.to_world[:] = _rows3x4(d.get("to_world")); e.radiance[:] = [float(v) for v in d["radiance"]]
            s.n_emitters = len(ems)
            s.emitters = C.cast(arr, C.POINTER(EmitterDesc))
            s._emitters_keep = arr                  # the list lives as long as the scene desc that points at it
        validate_rough(p)
        rough = p.boundary_bsdf == P.BSDF_HROUGHDIELECTRIC
        s.rough_distribution = p.rough_distribution if rough else 0
        s.rough_alpha = max(float(p.rough_alpha), 1e-4) if rough else 0.0
        s.rough_sample_visible = int(bool(p.rough_sample_visible) and p.rough_distribution != P.MICROFACET_PHONG) if rough else 0
        return s

    def upload_scene(self, p, layout=LAYOUT_DENSE, rif_layout=None):
        """Uploads the numpy fields referenced by p and returns (SceneDesc, [Volume...])."""
        vols = []
        dens = alb = rif = None
        if p.sigma_mode == P.SIGMA_GRID and p.density is not None:
            dl = LAYOUT_CELL8 if layout in (LAYOUT_BRICK27, LAYOUT_BRICK125, LAYOUT_AUTO) else layout   # bricks are the RIF's layout; sigma_t keeps its cell records
            dens = self.upload_volume(p.density, p.density_aabb[0], p.density_aabb[1], dl if np.asarray(p.density).dtype != np.uint8 else LAYOUT_DENSE, p.density_to_world)
            vols.append(dens)
        if p.albedo_mode == P.ALBEDO_GRID and p.albedo_grid is not None:
            alb = self.upload_volume(p.albedo_grid, p.albedo_aabb[0], p.albedo_aabb[1], to_world=p.albedo_to_world)
            vols.append(alb)
        if p.rif_mode not in (P.RIF_CONST, P.RIF_ACOUSTIC) and p.rif is not None:
            rl = layout if rif_layout is None else rif_layout
            rif = self.upload_volume(p.rif, p.rif_aabb[0], p.rif_aabb[1], rl if p.rif_mode == P.RIF_TRILINEAR else LAYOUT_DENSE, p.rif_to_world)
            if p.rif_mode == P.RIF_BSPLINE3:
                rif.build_spline()
            vols.append(rif)
        sdf = None
        if p.boundary == P.BOUNDARY_SDF and p.sdf is not None:
            sdf = self.upload_volume(p.sdf, p.sdf_aabb[0], p.sdf_aabb[1], LAYOUT_DENSE, p.sdf_to_world)
            vols.append(sdf)
        env = _upload_scene_envmap(self, p, vols)
        return self.scene_desc(p, dens, alb, rif, sdf, env), vols

    def upload_envmap(self, image):
        """mer_envmap_upload: the lat-long image float [height][width][3] -> a Volume handle (freed by destroy / mer_volume_destroy)"""
        a = np.ascontiguousarray(np.asarray(image, np.float32))
        if a.ndim != 3 or a.shape[2] != 3:
            raise MerError("envmap emitter: the image must be float [height][width][3]")
        h = C.c_int32()
        self._check(self.lib.mer_envmap_upload(self.h, C.c_int32(a.shape[1]), C.c_int32(a.shape[0]), _fp(a), C.byref(h)))
        return Volume(self, h.value, None, None)

    # ---- film + render -------------------------------------------------------------------------
    def film_channels(self, scene):
        """frames*3 + 2: RGB per frame, alpha, weight (5 in steady state)"""
        ch = C.c_int32()
        self._check(self.lib.mer_film_channels(self.h, C.byref(scene), C.byref(ch)))
        return ch.value

    def film_alloc(self, w, h, channels=5):
        ptr = C.c_void_p()
        self._check(self.lib.mer_film_alloc_n(self.h, C.c_int32(w), C.c_int32(h), C.c_int32(channels), C.byref(ptr)))
        return ptr

    def film_zero(self, ptr, w, h, channels=5):
        self._check(self.lib.mer_film_zero_n(self.h, ptr, C.c_int32(w), C.c_int32(h), C.c_int32(channels)))

    def film_download(self, ptr, w, h, channels=5):
        out = np.empty((h, w, channels), np.float32)
        self._check(self.lib.mer_film_download_n(self.h, ptr, C.c_int32(w), C.c_int32(h), C.c_int32(channels), _fp(out)))
        return out

    def film_free(self, ptr):
        self._check(self.lib.mer_film_free(self.h, ptr))

    def render(self, scene, film_ptr, spp_begin, spp_count, seed=0, spp_stride=1, tile_rank=0, tile_count=1):
        """Asynchronous on the context stream.  film_ptr: c_void_p / int device pointer."""
        sh = Shard(spp_begin, spp_count, spp_stride, tile_rank, tile_count)
        fp = film_ptr if isinstance(film_ptr, C.c_void_p) else C.c_void_p(int(film_ptr))
        self._check(self.lib.mer_render(self.h, C.byref(scene), C.byref(sh), C.c_uint64(seed), fp))

    def render_to_host(self, scene, spp_begin, spp_count, seed=0, **kw):
        ch = self.film_channels(scene)
        f = self.film_alloc(scene.width, scene.height, ch)
        try:
            self.render(scene, f, spp_begin, spp_count, seed, **kw)
            return self.film_download(f, scene.width, scene.height, ch)
        finally:
            self.film_free(f)

    # ---- what light paths record: fluence grids, exitance maps, sensitivity grids (one implementation over _RECORDERS) ----
    def _recorder_create(self, kind, *args):
        k = _RECORDERS[kind]
        d = k.desc(*args)
        k.validate(d)
        h = C.c_int32()
        self._check(getattr(self.lib, k.create)(self.h, C.byref(d), C.byref(h)))
        self._recorders[h.value] = (kind, k.shape(d))
        return h.value

    def _recorder_clear(self, family, handle):
        self._check(getattr(self.lib, "mer_%s_clear" % family)(self.h, C.c_int32(handle)))

    def _recorder_destroy(self, family, handle):
        self._check(getattr(self.lib, "mer_%s_destroy" % family)(self.h, C.c_int32(handle)))
        self._recorders.pop(handle, None)

    def _recorder_render(self, family, scene, handle, spp_begin, spp_count, seed, spp_stride, tile_rank, tile_count):
        sh = Shard(spp_begin, spp_count, spp_stride, tile_rank, tile_count)
        self._check(getattr(self.lib, "mer_render_%s" % family)(self.h, C.byref(scene), C.byref(sh), C.c_uint64(seed), C.c_int32(handle)))

    def _recorder_read(self, kind, handle, sums):
        """the read entry point of `kind` on the handle: (sums or None, totals).  The shape is the handle's own; one of another family, or of
        the family's other read, is refused here as the library refuses it"""
        k = _RECORDERS[kind]
        totals = np.zeros(k.totals, np.float64)
        out = None
        if sums:
            mine, shape = self._recorders.get(handle, (None, None))
            if mine is None or _RECORDERS[mine].family != k.family:
                raise MerError("%s: unknown %s handle" % (k.read, k.family))
            if _RECORDERS[mine].read != k.read:
                raise MerError("%s: %s: use %s" % (k.read, _RECORDERS[mine].what, _RECORDERS[mine].read))
            out = np.zeros(shape + (3,), np.float64)
        self._check(getattr(self.lib, k.read)(self.h, C.c_int32(handle), _fp(out) if sums else None, _fp(totals)))
        return out, totals

    # ---- the fluence grid recorded from light paths (mer_render_fluence) ------------------------
    def fluence_create(self, res, bmin, bmax):
        """-> handle of a zeroed grid of res = (nx, ny, nz) cells over the box bmin ... bmax"""
        return self._recorder_create("fluence", res, bmin, bmax)

    def fluence_track_create(self, res, bmin, bmax):
        """-> handle of a zeroed track-length grid (mer_fluence_track_create): the layout of fluence_create, filled by the track-length
        estimator.  fluence_clear, fluence_destroy, render_fluence and fluence_read take it like a fluence_create handle."""
        return self._recorder_create("fluence_track", res, bmin, bmax)

    def fluence_time_create(self, res, bmin, bmax, frames, t_min, t_bin):
        """-> handle of a zeroed time-resolved grid: the box of fluence_create, `frames` bins of width t_bin from t_min on in optical path
        length.  fluence_clear, fluence_destroy and render_fluence take it like any other fluence handle."""
        return self._recorder_create("fluence_time", res, bmin, bmax, frames, t_min, t_bin)

    def fluence_clear(self, handle):
        self._recorder_clear("fluence", handle)

    def fluence_destroy(self, handle):
        self._recorder_destroy("fluence", handle)

    def render_fluence(self, scene, handle, spp_begin, spp_count, seed=0, spp_stride=1, tile_rank=0, tile_count=1):
        """accumulates the light paths of the shard into the grid; returns synchronised"""
        self._recorder_render("fluence", scene, handle, spp_begin, spp_count, seed, spp_stride, tile_rank, tile_count)

    def fluence_read(self, handle, sums=True):
        """-> (raw sums float64 [nz][ny][nx][3], or None with sums = False; totals float64 [8])"""
        return self._recorder_read("fluence", handle, sums)

    def fluence_time_read(self, handle, sums=True):
        """-> (raw sums float64 [frames][nz][ny][nx][3], or None with sums = False; totals float64 [12])"""
        return self._recorder_read("fluence_time", handle, sums)

    def fluence_fd_create(self, res, bmin, bmax, wavenumbers):
        """-> handle of a zeroed frequency-domain grid (mer_fluence_fd_create): the box of fluence_create and up to 8 wavenumbers k >= 0 in
        radians per unit of optical path length (2 pi f / c0; 0: the steady state).  fluence_clear, fluence_destroy and render_fluence take it
        like any other fluence handle."""
        return self._recorder_create("fluence_fd", res, bmin, bmax, wavenumbers)

    def fluence_fd_read(self, handle, sums=True):
        """-> (raw float64 sums [n_freq][2][nz][ny][nx][3] -- real and imaginary plane per wavenumber -- or None, totals float64 [8]:
        capi.FLUENCE_TOTALS).  complex fluence = sums / (paths x cell volume)"""
        return self._recorder_read("fluence_fd", handle, sums)

    def _fluence_box(self, scene, bmin, bmax):
        """the box of a fluence map: the caller's, or the bounding box of the medium shape"""
        if bmin is None or bmax is None:
            if scene.boundary == P.BOUNDARY_SPHERE:
                c, r = np.array(scene.sph_center[:], np.float64), float(scene.sph_radius)
                lo, hi = c - r, c + r
            else:
                lo, hi = np.array(scene.bmin[:], np.float64), np.array(scene.bmax[:], np.float64)
            bmin = lo if bmin is None else bmin
            bmax = hi if bmax is None else bmax
        return bmin, bmax

    def fluence_time(self, scene, res, frames, t_min, t_bin, spp_count, seed=0, bmin=None, bmax=None):
        """One time-resolved fluence map of the scene (integrator = ptracer): (phi float64 [frames][nz][ny][nx][3], info).
        phi = sums / (paths x cell volume x t_bin), per unit of optical path length (divide the path length by c to get time) and of the
        emitters' intensity / power; the box defaults to the bounding box of the medium shape.  info: as Context.fluence has it, plus
        out_of_window [3] (the weight of deposits inside the box but outside the window), frames, t_min and t_bin."""
        bmin, bmax = self._fluence_box(scene, bmin, bmax)
        h = self.fluence_time_create(res, bmin, bmax, frames, t_min, t_bin)
        try:
            self.render_fluence(scene, h, 0, spp_count, seed)
            sums, t = self.fluence_time_read(h)
        finally:
            self.fluence_destroy(h)
        d = fluence_time_desc(res, bmin, bmax, frames, t_min, t_bin)
        volume = float(np.prod([(np.float64(d.bmax[a]) - np.float64(d.bmin[a])) / d.res[a] for a in range(3)]))
        info = {"paths": t[0], "escaped": t[1:4].copy(), "dropped": t[4:7].copy(), "ended": t[7], "out_of_window": t[8:11].copy(), "sums": sums,
                "bmin": np.array(d.bmin[:], np.float64), "bmax": np.array(d.bmax[:], np.float64), "cell_volume": volume,
                "frames": d.frames, "t_min": float(d.t_min), "t_bin": float(d.t_bin)}
        phi = sums / (t[0] * volume * np.float64(d.t_bin)) if t[0] > 0 else np.zeros_like(sums)
        return phi, info

    def fluence(self, scene, res, spp_count, seed=0, bmin=None, bmax=None, spp_begin=0, estimator="collision"):
        """One fluence map of the scene (integrator = ptracer): (phi float64 [nz][ny][nx][3], info).  phi = sums / (paths x cell volume), per
        unit of the emitters' intensity / power; the box defaults to the bounding box of the medium shape.  info: the totals by name
        (paths, escaped [3], dropped [3], ended), the raw sums, the box, the cell volume and the estimator.
        estimator: "collision" (one deposit per real collision) or "track" (every free flight deposits along its path, voids included;
        needs analog distance sampling: mer.h, mer_fluence_track_create)."""
        if estimator not in ("collision", "track"):
            raise MerError("fluence: estimator must be \"collision\" or \"track\"")
        bmin, bmax = self._fluence_box(scene, bmin, bmax)
        h = self.fluence_track_create(res, bmin, bmax) if estimator == "track" else self.fluence_create(res, bmin, bmax)
        try:
            self.render_fluence(scene, h, spp_begin, spp_count, seed)
            sums, t = self.fluence_read(h)
        finally:
            self.fluence_destroy(h)
        d = fluence_desc(res, bmin, bmax)
        volume = float(np.prod([(np.float64(d.bmax[a]) - np.float64(d.bmin[a])) / d.res[a] for a in range(3)]))
        info = {"paths": t[0], "escaped": t[1:4].copy(), "dropped": t[4:7].copy(), "ended": t[7], "sums": sums,
                "bmin": np.array(d.bmin[:], np.float64), "bmax": np.array(d.bmax[:], np.float64), "cell_volume": volume, "estimator": estimator}
        phi = sums / (t[0] * volume) if t[0] > 0 else np.zeros_like(sums)
        return phi, info

    # ---- the exitance map recorded from light paths (mer_render_exitance) -----------------------
    def exitance_create(self, boundary, res, frames=1, t_min=0.0, t_bin=0.0, cos_min=0.0):
        """-> handle of a zeroed map of res = (res_u, res_v) cells on every face of the boundary (P.BOUNDARY_AABB: 6, P.BOUNDARY_SPHERE: 1)"""
        return self._recorder_create("exitance", boundary, res, frames, t_min, t_bin, cos_min)

    def exitance_clear(self, handle):
        self._recorder_clear("exitance", handle)

    def exitance_destroy(self, handle):
        self._recorder_destroy("exitance", handle)

    def render_exitance(self, scene, handle, spp_begin, spp_count, seed=0, spp_stride=1, tile_rank=0, tile_count=1):
        """accumulates the exits of the shard's light paths into the map; returns synchronised"""
        self._recorder_render("exitance", scene, handle, spp_begin, spp_count, seed, spp_stride, tile_rank, tile_count)

    def exitance_read(self, handle, sums=True):
        """-> (raw sums float64 [frames][faces][res_v][res_u][3], or None with sums = False; totals float64 [16])"""
        return self._recorder_read("exitance", handle, sums)

    def exitance_fd_create(self, boundary, res, wavenumbers, cos_min=0.0):
        """-> handle of a zeroed frequency-domain map (mer_exitance_fd_create): the raster and cone of exitance_create and up to 8
        wavenumbers.  exitance_clear, exitance_destroy and render_exitance take it like any other exitance handle."""
        return self._recorder_create("exitance_fd", boundary, res, wavenumbers, cos_min)

    def exitance_fd_read(self, handle, sums=True):
        """-> (raw float64 sums [n_freq][2][faces][res_v][res_u][3] or None, totals float64 [16]: capi.EXITANCE_TOTALS; `late` stays 0).
        complex exitance = sums / (paths x cell area)"""
        return self._recorder_read("exitance_fd", handle, sums)

    def exitance(self, scene, res, spp_count, frames=1, t_min=0.0, t_bin=0.0, cos_min=0.0, seed=0, spp_begin=0):
        """One exitance map of the scene (integrator = ptracer) over the boundary of its medium shape: (raw sums float64
        [frames][faces][res_v][res_u][3], totals float64 [16]: capi.EXITANCE_TOTALS).  exitance = sums / (paths x cell area [x t_bin])."""
        h = self.exitance_create(scene.boundary, res, frames, t_min, t_bin, cos_min)
        try:
            self.render_exitance(scene, h, spp_begin, spp_count, seed)
            return self.exitance_read(h)
        finally:
            self.exitance_destroy(h)

    # ---- the sensitivity grid of a detector on the boundary (mer_render_sensitivity) ------------
    def sensitivity_create(self, res, bmin, bmax, detector):
        """-> handle of a zeroed grid of res = (nx, ny, nz) cells over the box bmin ... bmax for the detector (capi.detector_desc)"""
        return self._recorder_create("sensitivity", res, bmin, bmax, detector)

    def sensitivity_clear(self, handle):
        self._recorder_clear("sensitivity", handle)

    def sensitivity_destroy(self, handle):
        self._recorder_destroy("sensitivity", handle)

    def render_sensitivity(self, scene, handle, spp_begin, spp_count, seed=0, spp_stride=1, tile_rank=0, tile_count=1):
        """accumulates w x length of the shard's detected light paths into the grid; returns synchronised"""
        self._recorder_render("sensitivity", scene, handle, spp_begin, spp_count, seed, spp_stride, tile_rank, tile_count)

    def sensitivity_read(self, handle, sums=True):
        """-> (raw sums float64 [nz][ny][nx][3], or None with sums = False; totals float64 [16]: capi.SENSITIVITY_TOTALS)"""
        mine, shape = self._recorders.get(handle, (None, None))
        if mine != "sensitivity_array":
            return self._recorder_read("sensitivity", handle, sums)
        # a handle of sensitivity_array_create: the library takes it with one measurement and no K, and refuses it by name otherwise
        totals = np.zeros(16, np.float64)
        single = shape[:4] == (1, 1, 1, 1)
        out = np.zeros(shape[4:] + (3,), np.float64) if sums and single else None
        self._check(self.lib.mer_sensitivity_read(self.h, C.c_int32(handle), _fp(out) if out is not None else None, _fp(totals)))
        return out, totals

    # ---- detector arrays, gates and the scattering grid (mer_sensitivity_array_create) ----------
    def sensitivity_array_create(self, res, bmin, bmax, detector, bins=None, gates=1, scatter=False):
        """-> handle of the zeroed grids of an array of detectors: one detector is bins = (bin_u, bin_v) raster cells of the detector's window
        (None: all of it), gate g takes the exits with floor((l - t_min) / t_bin) == g for 0 <= g < gates; scatter: the scattering grids K too.
        sensitivity_clear, sensitivity_destroy and render_sensitivity take it like a sensitivity_create handle."""
        return self._recorder_create("sensitivity_array", res, bmin, bmax, detector, bins, gates, scatter)

    def sensitivity_shape(self, handle):
        """-> (gates, ndv, ndu, scatter) of a handle of sensitivity_create or sensitivity_array_create"""
        shape = (C.c_int32 * 4)()
        self._check(self.lib.mer_sensitivity_shape(self.h, C.c_int32(handle), shape))
        return tuple(int(v) for v in shape)

    def sensitivity_read_array(self, handle, sums=True):
        """-> (raw sums float64 [1 + scatter][gates][ndv][ndu][nz][ny][nx][3], or None with sums = False; meas float64 [gates][ndv][ndu][8]:
        detected weight x 3, detected paths, w x scattering collisions x 3, 0; totals float64 [16]: capi.SENSITIVITY_ARRAY_TOTALS)"""
        mine, shape = self._recorders.get(handle, (None, None))
        if mine not in ("sensitivity", "sensitivity_array"):
            raise MerError("mer_sensitivity_read_array: unknown sensitivity handle")
        if mine == "sensitivity":
            shape = (1, 1, 1, 1) + shape
        out = np.zeros(shape + (3,), np.float64) if sums else None
        meas = np.zeros(shape[1:4] + (8,), np.float64)
        totals = np.zeros(16, np.float64)
        self._check(self.lib.mer_sensitivity_read_array(self.h, C.c_int32(handle), _fp(out) if sums else None, _fp(meas), _fp(totals)))
        return out, meas, totals

    def sensitivity_array(self, scene, res, detector, bins, gates, spp_count, scatter=False, seed=0, bmin=None, bmax=None, spp_begin=0):
        """The sensitivity maps of an array of detectors and gates in one render (integrator = ptracer): (J / paths float64
        [gates][ndv][ndu][nz][ny][nx][3], K / paths of the same shape or None without scatter, meas float64 [gates][ndv][ndu][8], info).
        detector: capi.detector_desc or a dict of its arguments without the boundary; its (t_min, t_bin) is gate 0.  In a medium with
        homogeneous sigma_s the derivative of the detected signal of measurement m by sigma_s is sum(K[m]) / sigma_s - sum(J[m]) per
        channel (per cell: K_c / sigma_s - J_c); with a gridded sigma_t or albedo K is raw: w per scattering collision.  info: the totals
        by name (as Context.sensitivity, plus collisions_dropped [3]), the raw sums [1 + scatter][...] and the box."""
        if isinstance(detector, dict):
            detector = detector_desc(scene.boundary, **detector)
        bmin, bmax = self._fluence_box(scene, bmin, bmax)
        h = self.sensitivity_array_create(res, bmin, bmax, detector, bins, gates, scatter)
        try:
            self.render_sensitivity(scene, h, spp_begin, spp_count, seed)
            sums, meas, t = self.sensitivity_read_array(h)
        finally:
            self.sensitivity_destroy(h)
        d = fluence_desc(res, bmin, bmax)
        info = {"paths": t[0], "detected_weight": t[1:4].copy(), "dropped": t[4:7].copy(), "ended": t[7], "detected": t[8],
                "weight_length": t[9:12].copy(), "disagreements": t[12], "collisions_dropped": t[13:16].copy(), "sums": sums, "totals": t,
                "bmin": np.array(d.bmin[:], np.float64), "bmax": np.array(d.bmax[:], np.float64)}
        scaled = sums / t[0] if t[0] > 0 else np.zeros_like(sums)
        return scaled[0], (scaled[1] if scatter else None), meas, info

    def sensitivity(self, scene, res, detector, spp_count, seed=0, bmin=None, bmax=None, spp_begin=0):
        """One sensitivity map of the scene (integrator = ptracer) for a detector on the boundary of its medium shape (capi.detector_desc,
        or a dict of its arguments without the boundary): (J / paths float64 [nz][ny][nx][3], info).  With S = detected weight / paths the
        detected signal, dS / d sigma_a of cell c is -J_c / paths, whatever the distance sampling; J_c / detected weight is the mean
        partial path length in c.  The box defaults to the bounding box of the medium shape.  info: the totals by name (paths,
        detected_weight [3], dropped [3], ended, detected, weight_length [3], disagreements), the raw sums and the box."""
        if isinstance(detector, dict):
            detector = detector_desc(scene.boundary, **detector)
        bmin, bmax = self._fluence_box(scene, bmin, bmax)
        h = self.sensitivity_create(res, bmin, bmax, detector)
        try:
            self.render_sensitivity(scene, h, spp_begin, spp_count, seed)
            sums, t = self.sensitivity_read(h)
        finally:
            self.sensitivity_destroy(h)
        d = fluence_desc(res, bmin, bmax)
        info = {"paths": t[0], "detected_weight": t[1:4].copy(), "dropped": t[4:7].copy(), "ended": t[7], "detected": t[8],
                "weight_length": t[9:12].copy(), "disagreements": t[12], "sums": sums, "totals": t,
                "bmin": np.array(d.bmin[:], np.float64), "bmax": np.array(d.bmax[:], np.float64)}
        return (sums / t[0] if t[0] > 0 else np.zeros_like(sums)), info

    def synchronize(self):
        self._check(self.lib.mer_synchronize(self.h))

    def last_kernel_ms(self):
        ms = C.c_float()
        self._check(self.lib.mer_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    def last_render_stats(self):
        n = C.c_int32(); a = C.c_float(); b = C.c_float()
        self._check(self.lib.mer_last_render_stats(self.h, C.byref(n), C.byref(a), C.byref(b)))
        return n.value, a.value, b.value

    def counters(self):
        out = np.zeros(C_COUNT, np.uint64)
        self._check(self.lib.mer_counters_read(self.h, _fp(out)))
        return out

    def counters_reset(self):
        self._check(self.lib.mer_counters_reset(self.h))

    # ---- leaf entry points ---------------------------------------------------------------------
    def lookup_trilinear(self, vol, pts):
        pts = _f32(pts); n = pts.shape[0]
        val = np.empty(n, np.float32); idx = np.empty((n, 4), np.int32)
        self._check(self.lib.mer_lookup_trilinear(self.h, C.c_int32(vol.handle), _fp(pts), C.c_int64(n), _fp(val), _fp(idx)))
        return val, idx

    def lookup_trilinear_rgb(self, vol, pts):
        pts = _f32(pts); n = pts.shape[0]
        out = np.empty((n, 3), np.float32)
        self._check(self.lib.mer_lookup_trilinear_rgb(self.h, C.c_int32(vol.handle), _fp(pts), C.c_int64(n), _fp(out)))
        return out

    def rif_value_grad(self, vol, interp, pts):
        pts = _f32(pts); n = pts.shape[0]
        val = np.empty(n, np.float32); grad = np.empty((n, 3), np.float32)
        self._check(self.lib.mer_rif_value_grad(self.h, C.c_int32(vol.handle), C.c_int32(interp), _fp(pts), C.c_int64(n), _fp(val), _fp(grad)))
        return val, grad

    def acoustic_value_grad(self, scene, pts):
        """the scene's analytic acoustic RIF (rif_mode = RIF_ACOUSTIC) and its gradient at pts"""
        pts = _f32(pts); n = pts.shape[0]
        val = np.empty(n, np.float32); grad = np.empty((n, 3), np.float32)
        self._check(self.lib.mer_acoustic_value_grad(self.h, C.byref(scene), _fp(pts), C.c_int64(n), _fp(val), _fp(grad)))
        return val, grad

    def er_trace(self, scene, p0, d0, dist):
        p0 = _f32(p0); d0 = _f32(d0); dist = _f32(dist); n = p0.shape[0]
        op = np.empty((n, 3), np.float32); ov = np.empty((n, 3), np.float32)
        ds = np.empty(n, np.float32); oo = np.empty(n, np.float32); ok = np.empty(n, np.int32)
        self._check(self.lib.mer_er_trace(self.h, C.byref(scene), _fp(p0), _fp(d0), _fp(dist), C.c_int64(n),
                                       _fp(op), _fp(ov), _fp(ds), _fp(oo), _fp(ok)))
        return op, ov, ds, oo, ok

    def sample_distance(self, scene, o, d, maxt, seed):
        o = _f32(o); d = _f32(d); maxt = _f32(maxt); n = o.shape[0]
        rec = np.empty((n, 20), np.float32)
        self._check(self.lib.mer_sample_distance(self.h, C.byref(scene), _fp(o), _fp(d), _fp(maxt), C.c_int64(n), C.c_uint64(seed), _fp(rec)))
        return rec

    def connect(self, scene, p1, p2, seed):
        p1 = _f32(p1); p2 = _f32(p2); n = p1.shape[0]
        out = np.zeros((n, 12), np.float32)
        self._check(self.lib.mer_connect(self.h, C.byref(scene), _fp(p1), _fp(p2), C.c_int64(n), C.c_uint64(seed), _fp(out)))
        return out

    def envmap_eval(self, scene, dirs):
        """mer_envmap_eval: the scene's envmap at world directions dirs (n x 3) -> (value x scale (n, 3), pdfDirect (n,))"""
        d = _f32(dirs).reshape(-1, 3); n = d.shape[0]
        val = np.zeros((n, 3), np.float32); pdf = np.zeros(n, np.float32)
        self._check(self.lib.mer_envmap_eval(self.h, C.byref(scene), _fp(d), C.c_int64(n), _fp(val), _fp(pdf)))
        return val, pdf

    def envmap_sample(self, scene, u2):
        """mer_envmap_sample: sampleDirect for samples u2 (n x 2) -> (direction (n, 3), value / pdf (n, 3), pdf (n,))"""
        u = _f32(u2).reshape(-1, 2); n = u.shape[0]
        d = np.zeros((n, 3), np.float32); v = np.zeros((n, 3), np.float32); pdf = np.zeros(n, np.float32)
        self._check(self.lib.mer_envmap_sample(self.h, C.byref(scene), _fp(u), C.c_int64(n), _fp(d), _fp(v), _fp(pdf)))
        return d, v, pdf

    def emitter_direct(self, scene, k, ref):
        """mer_emitter_direct: sampleDirect of emitter-list entry k (a point or a spot) at the reference points ref (n x 3); (n, 8) float32:
        value RGB (not divided by the selection pdf), unit direction to the emitter, distance, falloff"""
        ref = _f32(ref).reshape(-1, 3); n = ref.shape[0]
        out = np.zeros((n, 8), np.float32)
        self._check(self.lib.mer_emitter_direct(self.h, C.byref(scene), C.c_int32(k), _fp(ref), C.c_int64(n), _fp(out)))
        return out

    def area_direct(self, scene, k, ref, u2):
        """mer_area_direct: sampleDirect of emitter-list entry k (an area emitter on a rectangle, disk or sphere) at the reference points ref
        (n x 3) with the samples u2 (n x 2); (n, 12) float32: radiance / pdf RGB (not divided by the selection pdf), d, dist, the solid-angle
        pdf, the normal at the sampled point, 0"""
        ref = _f32(ref).reshape(-1, 3); u = _f32(u2).reshape(-1, 2); n = ref.shape[0]
        if u.shape[0] != n:
            raise ValueError("area_direct: ref and u2 must have the same length")
        out = np.zeros((n, 12), np.float32)
        self._check(self.lib.mer_area_direct(self.h, C.byref(scene), C.c_int32(k), _fp(ref), _fp(u), C.c_int64(n), _fp(out)))
        return out

    def area_hit(self, scene, o, d, ref):
        """mer_area_hit: the nearest area-emitter shape along o + t d, t >= 0 (n x 3 each); (n, 8) float32: list index or -1, t, the radiance
        seen along d RGB, pdfDirect of the hit point from ref (solid angle, without the selection pdf), 0, 0"""
        o = _f32(o).reshape(-1, 3); d = _f32(d).reshape(-1, 3); ref = _f32(ref).reshape(-1, 3); n = o.shape[0]
        if d.shape[0] != n or ref.shape[0] != n:
            raise ValueError("area_hit: o, d and ref must have the same length")
        out = np.zeros((n, 8), np.float32)
        self._check(self.lib.mer_area_hit(self.h, C.byref(scene), _fp(o), _fp(d), _fp(ref), C.c_int64(n), _fp(out)))
        return out

    def eval_transmittance(self, scene, o, d, maxt, seed):
        o = _f32(o); d = _f32(d); maxt = _f32(maxt); n = o.shape[0]
        out = np.empty((n, 3), np.float32)
        self._check(self.lib.mer_eval_transmittance(self.h, C.byref(scene), _fp(o), _fp(d), _fp(maxt), C.c_int64(n), C.c_uint64(seed), _fp(out)))
        return out

    def phase_sample(self, kind, g, wi, u2):
        wi = _f32(wi); u2 = _f32(u2); n = wi.shape[0]
        wo = np.empty((n, 3), np.float32); pdf = np.empty(n, np.float32)
        self._check(self.lib.mer_phase_sample(self.h, C.c_int32(kind), C.c_float(g), _fp(wi), _fp(u2), C.c_int64(n), _fp(wo), _fp(pdf)))
        return wo, pdf

    def phase_eval(self, kind, g, wi, wo):
        wi = _f32(wi); wo = _f32(wo); n = wi.shape[0]
        val = np.empty(n, np.float32)
        self._check(self.lib.mer_phase_eval(self.h, C.c_int32(kind), C.c_float(g), _fp(wi), _fp(wo), C.c_int64(n), _fp(val)))
        return val

    def rough_eval(self, scene, eta, wi, wo):
        """mer_rough_dielectric_eval: f |cos theta_o| and pdf of the scene's rough_* microfacet dielectric, local frame, eta per item"""
        wi = _f32(wi); wo = _f32(wo); n = wi.shape[0]; eta = _f32(np.broadcast_to(np.asarray(eta, np.float32), (n,)))
        val = np.empty(n, np.float32); pdf = np.empty(n, np.float32)
        self._check(self.lib.mer_rough_dielectric_eval(self.h, C.byref(scene), _fp(eta), _fp(wi), _fp(wo), C.c_int64(n), _fp(val), _fp(pdf)))
        return val, pdf

    def rough_sample(self, scene, eta, wi, u3):
        """mer_rough_dielectric_sample: wo, weight = eval / pdf (0: no sample), pdf; u3 = microfacet 2D + reflect / refract choice"""
        wi = _f32(wi); u3 = _f32(u3); n = wi.shape[0]; eta = _f32(np.broadcast_to(np.asarray(eta, np.float32), (n,)))
        wo = np.empty((n, 3), np.float32); w = np.empty(n, np.float32); pdf = np.empty(n, np.float32)
        self._check(self.lib.mer_rough_dielectric_sample(self.h, C.byref(scene), _fp(eta), _fp(wi), _fp(u3), C.c_int64(n), _fp(wo), _fp(w), _fp(pdf)))
        return wo, w, pdf

    def camera_rays(self, scene, pos2):
        pos2 = _f32(pos2); n = pos2.shape[0]
        o = np.empty((n, 3), np.float32); d = np.empty((n, 3), np.float32)
        self._check(self.lib.mer_camera_rays(self.h, C.byref(scene), _fp(pos2), C.c_int64(n), _fp(o), _fp(d)))
        return o, d

    def sensor_rays(self, scene, pos2, aperture2=None):
        """mer_sensor_rays: o, d, mint, maxt of the scene's sensor kind; aperture2 = the aperture samples (the two lens kinds need them)"""
        pos2 = _f32(pos2); n = pos2.shape[0]
        ap = None if aperture2 is None else _f32(aperture2)
        if ap is not None and ap.shape != pos2.shape:
            raise MerError("sensor_rays: one aperture sample per film position")
        o = np.empty((n, 3), np.float32); d = np.empty((n, 3), np.float32); mint = np.empty(n, np.float32); maxt = np.empty(n, np.float32)
        self._check(self.lib.mer_sensor_rays(self.h, C.byref(scene), _fp(pos2), _fp(ap) if ap is not None else None, C.c_int64(n),
                                             _fp(o), _fp(d), _fp(mint), _fp(maxt)))
        return o, d, mint, maxt

    def sensor_direct(self, scene, ref):
        """mer_sensor_direct: PerspectiveCamera::sampleDirect at the points ref [n][3] -> [n][8]: value = importance / dist^2, film position
        (2), unit direction to the sensor (3), distance, 0; all zero outside the clip range or the frustum"""
        ref = _f32(ref); n = ref.shape[0]
        out = np.empty((n, 8), np.float32)
        self._check(self.lib.mer_sensor_direct(self.h, C.byref(scene), _fp(ref), C.c_int64(n), _fp(out)))
        return out

    def sensor_position(self, scene, dirs):
        """mer_sensor_position: getSamplePosition of the world directions dirs [n][3] -> (uv [n][2] in pixels, ok [n] bool)"""
        dirs = _f32(dirs); n = dirs.shape[0]
        uv = np.empty((n, 2), np.float32); ok = np.empty(n, np.int32)
        self._check(self.lib.mer_sensor_position(self.h, C.byref(scene), _fp(dirs), C.c_int64(n), _fp(uv), ok.ctypes.data_as(C.c_void_p)))
        return uv, ok != 0

    def correlation(self, scene, path_length):
        t = _f32(path_length); n = t.shape[0]
        out = np.empty(n, np.float32)
        self._check(self.lib.mer_correlation(self.h, C.byref(scene), _fp(t), C.c_int64(n), _fp(out)))
        return out

    def render_paths(self, scene, sample_index, seed=0):
        out = np.zeros((scene.height, scene.width, 3), np.float32)
        self._check(self.lib.mer_render_paths(self.h, C.byref(scene), C.c_int32(sample_index), C.c_uint64(seed), _fp(out)))
        return out

    def rng_floats(self, seed, pixel, sample, n):
        out = np.empty(n, np.float32)
        self._check(self.lib.mer_rng_floats(self.h, C.c_uint64(seed), C.c_uint32(pixel), C.c_uint32(sample), C.c_int32(n), _fp(out)))
        return out


class MultiContext:
    """Several GPUs in one process (include/mer.h: mer_multi_*): one context and, during a render, one host thread per listed device;
    volumes replicated; films sum-reduced onto the first device with RCCL (distinct devices) or peer copy + add (a device listed twice)."""

    def __init__(self, device_ids, check=False, **options):
        self.lib = lib(CHECK_LIB_PATH if check else None)
        ids = (C.c_int32 * len(device_ids))(*[int(d) for d in device_ids])
        self.h = C.c_void_p()
        if self.lib.mer_multi_create(ids, C.c_int32(len(device_ids)), C.byref(self.h)) != 0:
            raise MerError(self.lib.mer_multi_last_error(None).decode())
        self.device_ids = list(device_ids)
        self.contexts = [Context(d, check=check, _borrowed=self.lib.mer_multi_context(self.h, C.c_int32(i))) for i, d in enumerate(device_ids)]
        for k, v in options.items():
            self.set_option(k, v)

    def _check(self, rc):
        if rc != 0:
            raise MerError(self.lib.mer_multi_last_error(self.h).decode())

    def close(self):
        if self.h:
            self.lib.mer_multi_destroy(self.h)
            self.h = C.c_void_p()

    def set_option(self, name, value):
        self._check(self.lib.mer_multi_set_option(self.h, name.encode(), C.c_int64(int(value))))

    def upload_volume(self, data, aabb_min, aabb_max, layout=LAYOUT_DENSE, to_world=None):
        a = np.ascontiguousarray(data)
        if a.dtype != np.uint8:
            a = a.astype(np.float32, copy=False)
        ch = 1 if a.ndim == 3 else a.shape[3]
        d = Context._desc(a.shape, ch, P.VOL_U8 if a.dtype == np.uint8 else P.VOL_F32, aabb_min, aabb_max, to_world)
        h = C.c_int32()
        self._check(self.lib.mer_multi_volume_upload(self.h, C.byref(d), _fp(a), C.c_int32(layout), C.byref(h)))
        return Volume(self, h.value, d, layout)

    def upload_scene(self, p, layout=LAYOUT_DENSE):
        """the replicated-volume form of Context.upload_scene: every device receives every grid, one handle each"""
        vols = []
        dens = alb = rif = sdf = None
        if p.sigma_mode == P.SIGMA_GRID and p.density is not None:
            dl = LAYOUT_CELL8 if layout in (LAYOUT_BRICK27, LAYOUT_BRICK125, LAYOUT_AUTO) else layout
            dens = self.upload_volume(p.density, p.density_aabb[0], p.density_aabb[1], dl if np.asarray(p.density).dtype != np.uint8 else LAYOUT_DENSE, p.density_to_world)
            vols.append(dens)
        if p.albedo_mode == P.ALBEDO_GRID and p.albedo_grid is not None:
            alb = self.upload_volume(p.albedo_grid, p.albedo_aabb[0], p.albedo_aabb[1], to_world=p.albedo_to_world); vols.append(alb)
        if p.rif_mode not in (P.RIF_CONST, P.RIF_ACOUSTIC) and p.rif is not None:
            rif = self.upload_volume(p.rif, p.rif_aabb[0], p.rif_aabb[1], layout if p.rif_mode == P.RIF_TRILINEAR else LAYOUT_DENSE, p.rif_to_world)
            if p.rif_mode == P.RIF_BSPLINE3:
                self._check(self.lib.mer_multi_volume_build_spline(self.h, C.c_int32(rif.handle)))
            vols.append(rif)
        if p.boundary == P.BOUNDARY_SDF and p.sdf is not None:
            sdf = self.upload_volume(p.sdf, p.sdf_aabb[0], p.sdf_aabb[1], LAYOUT_DENSE, p.sdf_to_world); vols.append(sdf)
        env = _upload_scene_envmap(self, p, vols)
        return self.contexts[0].scene_desc(p, dens, alb, rif, sdf, env), vols

    def upload_envmap(self, image):
        """mer_multi_envmap_upload: one handle, valid in every context"""
        a = np.ascontiguousarray(np.asarray(image, np.float32))
        if a.ndim != 3 or a.shape[2] != 3:
            raise MerError("envmap emitter: the image must be float [height][width][3]")
        h = C.c_int32()
        self._check(self.lib.mer_multi_envmap_upload(self.h, C.c_int32(a.shape[1]), C.c_int32(a.shape[0]), _fp(a), C.byref(h)))
        return Volume(self, h.value, None, None)

    def destroy_volume(self, vol):
        if vol.handle:
            self._check(self.lib.mer_multi_volume_destroy(self.h, C.c_int32(vol.handle)))
            vol.handle = 0

    def render_to_host(self, scene, spp_begin, spp_count, seed=0, shard=SHARD_SAMPLES, rccl=1):
        ch = self.contexts[0].film_channels(scene)
        out = np.empty((scene.height, scene.width, ch), np.float32)
        self._check(self.lib.mer_multi_render(self.h, C.byref(scene), C.c_int32(shard), C.c_int32(spp_begin), C.c_int32(spp_count), C.c_uint64(seed),
                                              C.c_int32(rccl), _fp(out)))
        return out

    def last_stats(self):
        """-> (reduce path REDUCE_*, [render ms per context], reduce ms, counters summed over the contexts)"""
        path = C.c_int32(); ms = (C.c_float * len(self.contexts))(); red = C.c_float(); cnt = np.zeros(C_COUNT, np.uint64)
        self._check(self.lib.mer_multi_last_stats(self.h, C.byref(path), ms, C.byref(red), _fp(cnt)))
        return path.value, list(ms), red.value, cnt
