"""Flat scene parameters for the hot path (what the C-ABI descs carry).

Vocabulary follows the reference's plugins: a `heterogeneous` /
`homogeneous` / `heterogeneousrefractive` medium with `density` / `albedo` / `rif` volumes,
an `hg` / `isotropic` phase function, a `perspective` (or `orthographic` / `thinlens` /
`telecentric`) sensor with an `hdrfilm`, a
`volpath` integrator and a `constant` environment emitter.
"""
import numpy as np

# enums shared with include/mer.h
VOL_F32, VOL_U8 = 1, 3
SIGMA_HOMOGENEOUS, SIGMA_GRID = 0, 1
RIF_CONST, RIF_TRILINEAR, RIF_BSPLINE3 = 0, 1, 2
RIF_ACOUSTIC = 8          # acousticrifvolume, evaluated analytically: n_o + n_max J_m(k_r r) cos(m phi) in the (y, z) plane
STEP_VERLET, STEP_RK4 = 0, 1
BOUNDARY_AABB, BOUNDARY_SPHERE, BOUNDARY_SDF = 0, 1, 2
PHASE_ISOTROPIC, PHASE_HG = 0, 1
TR_WOODCOCK2, TR_RATIO = 0, 1
STRATEGY_BALANCE, STRATEGY_SINGLE, STRATEGY_MANUAL, STRATEGY_MAXIMUM = 0, 1, 2, 3
FILTER_BOX, FILTER_GAUSSIAN = 0, 1
ALBEDO_CONST, ALBEDO_GRID = 0, 1
DECOMPOSITION_NONE, DECOMPOSITION_TRANSIENT, DECOMPOSITION_BOUNCE = 0, 1, 2
METHOD_WOODCOCK, METHOD_SIMPSON = 0, 1
BSDF_NULL, BSDF_HDIELECTRIC, BSDF_HROUGHDIELECTRIC = 0, 1, 2
MICROFACET_BECKMANN, MICROFACET_GGX, MICROFACET_PHONG = 0, 1, 2
SENSOR_PERSPECTIVE, SENSOR_ORTHOGRAPHIC, SENSOR_THINLENS, SENSOR_TELECENTRIC = 0, 1, 2, 3      # src/sensors/: the projective family
INTEGRATOR_VOLPATH, INTEGRATOR_PTRACER = 0, 1          # path tracing from the sensor | light tracing (`ptracer`: paths start at an emitter)
MODULATION_NONE, MODULATION_SINE, MODULATION_SQUARE, MODULATION_HAMILTONIAN, MODULATION_MSEQ, MODULATION_DEPTHSELECTIVE = 0, 1, 2, 3, 4, 5


def look_at(origin, target, up):
    """Transform::lookAt (reference src/libcore/transform.cpp:191-214), float32, left-handed.
    Returns the row-major 3x4 camera-to-world matrix with columns (left, newUp, dir, origin)."""
    f = np.float32
    p = np.asarray(origin, f); t = np.asarray(target, f); u = np.asarray(up, f)
    d = (t - p).astype(f)
    d = (d / f(np.sqrt(f(np.dot(d, d))))).astype(f)
    left = np.cross(u, d).astype(f)
    left = (left / f(np.sqrt(f(np.dot(left, left))))).astype(f)
    new_up = np.cross(d, left).astype(f)
    m = np.zeros((3, 4), f)
    m[:, 0] = left; m[:, 1] = new_up; m[:, 2] = d; m[:, 3] = p
    return m


def world_to_volume(to_world):
    """inverse of a volume plugin's `toWorld` (GridDataSource::configure, src/volume/gridvolume.cpp:188-189) as the row-major 3x4
    float32 matrix the grid descs carry; None = identity (all zeros in the desc)."""
    if to_world is None:
        return np.zeros((3, 4), np.float32)
    m = np.eye(4); t = np.asarray(to_world, np.float64); m[:t.shape[0], :4] = t
    return np.linalg.inv(m)[:3, :4].astype(np.float32)


def rotation(axis, angle_deg, translate=(0, 0, 0)):
    """Transform::translate(t) * Transform::rotate(axis, angle) as a 4x4 (src/libcore/transform.cpp)"""
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a); th = np.deg2rad(angle_deg); c, s_ = np.cos(th), np.sin(th)
    x, y, z = a
    r = np.array([[c + x * x * (1 - c), x * y * (1 - c) - z * s_, x * z * (1 - c) + y * s_],
                  [y * x * (1 - c) + z * s_, c + y * y * (1 - c), y * z * (1 - c) - x * s_],
                  [z * x * (1 - c) - y * s_, z * y * (1 - c) + x * s_, c + z * z * (1 - c)]])
    m = np.eye(4); m[:3, :3] = r; m[:3, 3] = translate
    return m


class SceneParams:
    """Attribute bag; defaults follow the reference plugin defaults."""

    def __init__(self, **kw):
        # sensor perspective + film hdrfilm (scenes/volumetric/BoundedScatteringVolume_directionalsource.xml:27-49)
        self.width = 512; self.height = 512
        self.fov_x_deg = 95.8402; self.near_clip = 1e-2; self.far_clip = 1e4
        self.cam_to_world = look_at([-3, 0, 0], [-2, 0, 0], [0, 1, 0])
        # the sensor kind (SENSOR_*): orthographic / telecentric take the extent of their view from the scale in cam_to_world; thinlens and
        # telecentric have a world-space aperture_radius and a focus_distance (`apertureRadius`, `focusDistance`) and draw an aperture sample
        # after the pixel sample.  The defaults are the pinhole
        self.sensor = SENSOR_PERSPECTIVE; self.aperture_radius = 0.0; self.focus_distance = 0.0
        self.rfilter = FILTER_GAUSSIAN; self.rfilter_param = 0.5
        # integrator volpath (src/librender/integrator.cpp:190-225)
        self.max_depth = -1; self.rr_depth = 5; self.hide_emitters = False
        # INTEGRATOR_PTRACER: light tracing (src/integrators/ptracer): every scattering vertex of a path started at an emitter is connected
        # to the perspective sensor; emitters are list entries of kind point, spot or collimated (include/mer.h: mer_scene_desc.integrator)
        self.integrator = INTEGRATOR_VOLPATH
        # shape: cube [-1,1]^3 (scenes/volumetric/bounds.obj), null BSDF
        self.boundary = BOUNDARY_AABB
        self.boundary_bsdf = BSDF_NULL                            # BSDF_HDIELECTRIC: smooth dielectric, eta = RIF at the hit point
        # BSDF_HROUGHDIELECTRIC (src/bsdfs/hroughdielectric.cpp): its microfacet form -- distribution, isotropic alpha (clamped to >= 1e-4),
        # visible-normal sampling (off for phong)
        self.rough_distribution = MICROFACET_BECKMANN; self.rough_alpha = 0.1; self.rough_sample_visible = True
        self.bmin = [-1.0, -1.0, -1.0]; self.bmax = [1.0, 1.0, 1.0]
        self.sph_center = [0.0, 0.0, 0.0]; self.sph_radius = 1.0
        self.sdf = None; self.sdf_aabb = ([-1, -1, -1], [1, 1, 1])    # BOUNDARY_SDF: signed-distance grid, negative inside
        self.aggressive_tracing = False; self.sdf_max_error = None    # `aggressivetracing`: untested legs while deep inside the SDF shape;
        #                                                               None = the volume's maxSDFError(): one voxel diagonal (splinevolume.cpp:282)
        # medium
        self.sigma_mode = SIGMA_GRID
        self.sigma_a = [0.05, 0.05, 0.05]; self.sigma_s = [0.5, 3.5, 7.5]
        self.strategy = STRATEGY_BALANCE; self.channel = -1; self.sampling_density = 0.0
        self.medium_sampling_weight = -1.0
        self.density = None; self.density_aabb = ([-1, -1, -1], [1, 1, 1]); self.density_scale = 4.0
        # `toWorld` of the volume plugins (3x4 / 4x4, None = identity): src/volume/gridvolume.cpp:110,188-195
        self.density_to_world = None; self.albedo_to_world = None; self.rif_to_world = None; self.sdf_to_world = None
        self.albedo_mode = ALBEDO_CONST; self.albedo = [0.9, 0.9, 0.9]
        self.albedo_grid = None; self.albedo_aabb = ([-1, -1, -1], [1, 1, 1])
        self.rif_mode = RIF_CONST; self.rif_const = 1.0
        # RIF_ACOUSTIC (src/volume/acousticrifvolume.cpp:101-106): n_o, n_max, k_r = 2 pi freq / speed, mode
        self.ac_n_o = 1.3333; self.ac_n_max = 0.0; self.ac_k_r = 2.0 * 3.14159265358979323846 * 832000.0 / 1500.0; self.ac_mode = 0
        self.rif = None; self.rif_aabb = ([-1, -1, -1], [1, 1, 1])
        self.stepper = STEP_RK4; self.stepsize = 1e-3
        self.rif_double = 0
        self.phase = PHASE_HG; self.g = 0.8
        self.tr_estimator = TR_RATIO
        # heterogeneous `method` (woodcock | simpson) and its `stepSize` (0 = inferred from the grids): src/medium/heterogeneous.cpp:183-202,245-257
        self.method = METHOD_WOODCOCK; self.het_stepsize = 0.0
        self.env_radiance = [1.0, 1.0, 1.0]
        self.emission = [0.0, 0.0, 0.0]
        self.point_position = [0.0, 0.0, 0.0]; self.point_intensity = [0.0, 0.0, 0.0]     # emitter `point`
        # emitter `area` on a `rectangle` shape (src/emitters/area.cpp, src/shapes/rectangle.cpp): the image of [-1,1]^2 x {0} under area_to_world
        # (3x4 or 4x4, no shear; None = identity), radiance into the half space of its normal toWorld(0,0,1); zero radiance = none
        self.area_to_world = None; self.area_radiance = [0.0, 0.0, 0.0]
        # several point / area emitters (include/mer.h: mer_emitter): a list of point_emitter(...) / area_emitter(...) / disk_emitter(...) /
        # sphere_emitter(...) / spot_emitter(...) / envmap_emitter(...) entries.  Non-empty:
        # point_intensity and area_radiance must stay zero; one emitter of each kind is sampled per collision, chosen by samplingWeight
        self.emitters = []
        # film decomposition (src/librender/film.cpp:56-84): 0 none | 1 transient | 2 bounce (bins by edge count); frames = ceil((max-min)/binWidth)
        self.decomposition = DECOMPOSITION_NONE; self.min_bound = 0.0; self.max_bound = 0.0; self.bin_width = 1.0
        self.calibrated_transient = False
        # path-length modulation (src/librender/pathlengthsampler.cpp:12-40): lambda, phase [deg], P, neighbors
        self.modulation = MODULATION_NONE; self.mod_lambda = 1.0; self.mod_phase_deg = 0.0; self.mod_P = 32; self.mod_neighbors = 3
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError("unknown scene parameter '%s'" % k)
            setattr(self, k, v)

    def copy(self, **kw):
        q = SceneParams()
        q.__dict__.update(self.__dict__)
        for k, v in kw.items():
            if not hasattr(q, k):
                raise AttributeError("unknown scene parameter '%s'" % k)
            setattr(q, k, v)
        return q


EMITTER_POINT = 1
EMITTER_AREA = 2
EMITTER_SPOT = 3
EMITTER_ENVMAP = 4
EMITTER_AREA_DISK = 5
EMITTER_AREA_SPHERE = 6
EMITTER_COLLIMATED = 7
AREA_TYPES = (EMITTER_AREA, EMITTER_AREA_DISK, EMITTER_AREA_SPHERE)      # one kind: one selection CDF in list order
MAX_EMITTERS = 32


def point_emitter(position, intensity, sampling_weight=1.0):
    """an entry of SceneParams.emitters: emitter `point` (src/emitters/point.cpp) with its `samplingWeight`"""
    return {"type": EMITTER_POINT, "position": [float(v) for v in position], "intensity": [float(v) for v in intensity],
            "sampling_weight": float(sampling_weight)}


def area_emitter(to_world, radiance, sampling_weight=1.0):
    """an entry of SceneParams.emitters: emitter `area` on a `rectangle`, the image of [-1,1]^2 x {0} under to_world (3x4 or 4x4, no shear)"""
    return {"type": EMITTER_AREA, "to_world": to_world, "radiance": [float(v) for v in radiance], "sampling_weight": float(sampling_weight)}


def disk_emitter(to_world, radiance, sampling_weight=1.0):
    """an entry of SceneParams.emitters: emitter `area` on a `disk` (src/shapes/disk.cpp), the image of the unit disk in z = 0 under to_world
    (3x4 or 4x4, no shear, uniform u / v scale; a negative determinant is the reference's flipNormals); normal = to_world(Normal(0,0,1))"""
    return {"type": EMITTER_AREA_DISK, "to_world": to_world, "radiance": [float(v) for v in radiance], "sampling_weight": float(sampling_weight)}


def sphere_emitter(center, radius, radiance, sampling_weight=1.0, flip_normals=False):
    """an entry of SceneParams.emitters: emitter `area` on a `sphere` (src/shapes/sphere.cpp).  The entry carries the transform the C ABI reads:
    translate(center) * scale(radius), with the z scale negated for flip_normals (a negative determinant: the sphere emits inward)"""
    import numpy as np
    m = np.eye(4); r = float(radius)
    m[0, 0] = m[1, 1] = r; m[2, 2] = -r if flip_normals else r
    m[:3, 3] = [float(v) for v in center]
    return {"type": EMITTER_AREA_SPHERE, "to_world": m, "radiance": [float(v) for v in radiance], "sampling_weight": float(sampling_weight)}


def area_shape_error(kind, to_world):
    """why mer_render refuses the transform of a disk / sphere area emitter (None: accepted); the messages are the library's"""
    import numpy as np
    m = np.asarray(to_world if to_world is not None else np.eye(4), np.float64)
    if m.shape not in ((3, 4), (4, 4)) or not np.all(np.isfinite(m)):
        return "area emitter: 'toWorld' must be finite"
    A = m[:3, :3].astype(np.float32).astype(np.float64)
    if not abs(np.linalg.det(A)) > 0:
        return "area emitter: 'toWorld' is singular"
    l = np.sqrt((A * A).sum(axis=0))
    cos = lambda a, b: abs(float(np.dot(A[:, a], A[:, b])) / (l[a] * l[b]))
    if kind == EMITTER_AREA_DISK:
        if cos(0, 1) > 1e-3:
            return "Error: 'toWorld' transformation contains shear!"
        if abs(l[0] / l[1] - 1) > 1e-3:
            return "Error: 'toWorld' transformation contains a non-uniform scale!"
    elif kind == EMITTER_AREA_SPHERE:
        for a in range(3):
            b = (a + 1) % 3
            if abs(l[a] / l[b] - 1) > 1e-3 or cos(a, b) > 1e-3:
                return "sphere: 'toWorld' transformation contains a non-uniform scale!"
    return None


def spot_error(to_world, cutoff_deg, beam_deg):
    """why mer_render refuses a spot emitter with these parameters (None: accepted)"""
    import numpy as np
    c, b = float(cutoff_deg), float(beam_deg)
    if not (np.isfinite(c) and np.isfinite(b) and c >= 0 and b >= 0):
        return "spot emitter: cutoffAngle and beamWidth must be finite and non-negative"
    if c > 180:
        return "spot emitter: cutoffAngle must not exceed 180 degrees"
    if b > c:
        return "spot emitter: beamWidth must not exceed cutoffAngle"
    m = np.asarray(to_world if to_world is not None else np.eye(4), np.float64)
    if m.shape not in ((3, 4), (4, 4)) or not np.all(np.isfinite(m)):
        return "spot emitter: 'toWorld' must be a finite 3x4 or 4x4 transform"
    if not abs(np.linalg.det(m[:3, :3].astype(np.float32).astype(np.float64))) > 0:
        return "spot emitter: 'toWorld' is singular"
    return None


def spot_emitter(to_world, intensity, cutoff_deg=20.0, beam_deg=None, weight=1.0):
    """an entry of SceneParams.emitters: emitter `spot` (src/emitters/spot.cpp:66-118), a point emitter at to_world's origin whose cone
    axis is to_world's z axis; intensity is its peak intensity, cutoff_deg / beam_deg its `cutoffAngle` / `beamWidth` in degrees (beam
    defaults to 3/4 of the cutoff, in float as the reference computes it).  ValueError for what mer_render refuses."""
    import numpy as np
    if beam_deg is None:
        beam_deg = float(np.float32(cutoff_deg) * np.float32(3.0) / np.float32(4.0))
    err = spot_error(to_world, cutoff_deg, beam_deg)
    if err:
        raise ValueError(err)
    return {"type": EMITTER_SPOT, "to_world": to_world, "intensity": [float(v) for v in intensity],
            "cutoff_deg": float(cutoff_deg), "beam_deg": float(beam_deg), "sampling_weight": float(weight)}


def envmap_error(image, to_world, scale, sampling_weight):
    """why mer_render / mer_envmap_upload refuse an envmap emitter with these parameters (None: accepted).  The image checks are
    configure()'s (src/emitters/envmap.cpp:260-320) on the half-rounded texels."""
    import numpy as np
    a = np.asarray(image)
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        return "envmap emitter: the image must be float [height][width][3]"
    if max(a.shape[0], a.shape[1]) > 0xFFFF:
        return "Environment maps images must be smaller than 65536 pixels in width and height"
    with np.errstate(over="ignore", invalid="ignore"):
        h = a.astype(np.float32).astype(np.float16).astype(np.float32)
        lum = h[..., 0] * np.float32(0.212671) + h[..., 1] * np.float32(0.715160) + h[..., 2] * np.float32(0.072169)
    if not np.all(np.isfinite(lum)):
        return "The environment map contains an invalid floating point value (nan/inf) -- giving up."
    w = np.sin((np.arange(a.shape[0]) + 0.5) * np.pi / a.shape[0]).astype(np.float32)
    if not float(np.sum(lum.sum(axis=1, dtype=np.float64) * w)) != 0:
        return "The environment map is completely black -- this is not allowed."
    if not (np.isfinite(float(scale)) and float(scale) >= 0):
        return "envmap emitter: 'scale' must be finite and non-negative"
    if not (np.isfinite(float(sampling_weight)) and float(sampling_weight) > 0):
        return "samplingWeight must be positive"
    m = np.asarray(to_world if to_world is not None else np.eye(4), np.float64)
    if m.shape not in ((3, 4), (4, 4)) or not np.all(np.isfinite(m)):
        return "envmap emitter: 'toWorld' must be a finite 3x4 or 4x4 transform"
    R = m[:3, :3].astype(np.float32).astype(np.float64)
    if np.max(np.abs(R @ R.T - np.eye(3))) > 1e-5 or not np.linalg.det(R) > 0:
        return "envmap emitter: the linear part of 'toWorld' must be a rotation (within 1e-5)"
    return None


def envmap_emitter(image, to_world=None, scale=1.0, sampling_weight=1.0):
    """an entry of SceneParams.emitters: emitter `envmap` (src/emitters/envmap.cpp), the lat-long image float [height][width][3] (u = x
    along atan2(v.x, -v.z), v = y from the +y pole), its `toWorld` (a rotation; the translation is ignored), `scale` and `samplingWeight`.
    Context.upload_scene uploads the image (mer_envmap_upload).  The scene's env_radiance must be zero.  ValueError for what mer_render
    refuses."""
    import numpy as np
    a = np.ascontiguousarray(np.asarray(image, np.float32))
    err = envmap_error(a, to_world, scale, sampling_weight)
    if err:
        raise ValueError(err)
    return {"type": EMITTER_ENVMAP, "image": a, "to_world": to_world, "scale": float(scale), "sampling_weight": float(sampling_weight)}


def collimated_error(to_world):
    """why mer_render refuses a collimated emitter with this frame (None: accepted); the scale message is the reference's"""
    import numpy as np
    m = np.asarray(to_world if to_world is not None else np.eye(4), np.float64)
    if m.shape not in ((3, 4), (4, 4)) or not np.all(np.isfinite(m)):
        return "collimated emitter: 'toWorld' must be finite"
    R = m[:3, :3].astype(np.float32).astype(np.float64)
    if np.max(np.abs(R @ R.T - np.eye(3))) > 1e-4 or not np.linalg.det(R) > 0:
        return "Scale factors in the emitter-to-world transformation are not allowed!"
    return None


def collimated_emitter(to_world, power, sampling_weight=1.0):
    """an entry of SceneParams.emitters: emitter `collimated` (src/emitters/collimated.cpp), a beam that is a delta in position and
    direction: it starts at to_world's origin and runs along to_world's z axis (a 3x4 / 4x4 frame without scale: look_at gives one) and
    carries `power`.  Only light tracing (integrator = INTEGRATOR_PTRACER) can render it.  ValueError for what mer_render refuses."""
    err = collimated_error(to_world)
    if err:
        raise ValueError(err)
    return {"type": EMITTER_COLLIMATED, "to_world": to_world, "power": [float(v) for v in power], "sampling_weight": float(sampling_weight)}


def spot_position(e):
    """the position of a spot entry: the translation column of its to_world"""
    import numpy as np
    m = np.asarray(e.get("to_world") if e.get("to_world") is not None else np.eye(4), np.float64)
    return [float(np.float32(v)) for v in m[:3, 3]]


def sdf_max_error(p):
    """maxSDFError() of the scene's signed-distance volume: the diagonal of one voxel (src/volume/splinevolume.cpp:282), unless given."""
    if p.sdf_max_error is not None:
        return float(p.sdf_max_error)
    if p.sdf is None:
        return 0.0
    import numpy as np
    nz, ny, nx = np.asarray(p.sdf).shape[:3]
    lo, hi = np.asarray(p.sdf_aabb[0], np.float64), np.asarray(p.sdf_aabb[1], np.float64)
    st = (hi - lo) / np.array([nx - 1, ny - 1, nz - 1], np.float64)
    return float(np.sqrt((st * st).sum()))
