/*
 * mer.h -- C-ABI of libmer.so: the MI355X-native refractive volumetric path-tracing hot path.
 *
 * This is the drop-in boundary.  The reference (cmu-ci-lab/MitsubaER) has no
 * C-ABI for this path: its plugins are C++ classes behind `extern "C" CreateInstance(const Properties&)`
 * (include/mitsuba/core/cobject.h:99-107).  Each entry point below names the reference interface it
 * replaces.  Signatures use plain pointers, sizes and POD structs only -- no C++ / torch types.
 *
 * Conventions: every call returns 0 on success, non-zero on failure (reference: Log(EError) throws
 * std::runtime_error, src/libcore/logger.cpp:100-147; the message is kept for mer_last_error()).
 * The caller owns host buffers; the library owns device buffers behind handles.  One context per
 * (process, GPU); a context is single-threaded.  Grids are dense, x fastest:
 * data[((z*yres+y)*xres+x)*channels+c] (VOL v3 payload order, src/volume/gridvolume.cpp:54-89).
 * Pointers named *_dev are DEVICE pointers (e.g. a torch tensor's data_ptr()); all others are host.
 */
#ifndef MER_H
#define MER_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MER_ABI_VERSION 3

typedef struct mer_context mer_context;
typedef int32_t mer_volume;            /* handle, > 0; 0 = none */

/* VOL v3 type codes (src/volume/gridvolume.cpp:54-89) */
enum { MER_VOL_F32 = 1, MER_VOL_U8 = 3 };
enum { MER_SIGMA_HOMOGENEOUS = 0, MER_SIGMA_GRID = 1 };       /* medium `homogeneous` | `heterogeneous` */
enum { MER_RIF_CONST = 0, MER_RIF_TRILINEAR = 1, MER_RIF_BSPLINE3 = 2,   /* none | gridvolume | splinevolume */
       MER_RIF_ACOUSTIC = 8 };   /* acousticrifvolume: analytic, no grid (values 3..7 are internal fetch kinds of the trilinear RIF) */
enum { MER_STEP_VERLET = 0, MER_STEP_RK4 = 1 };
enum { MER_BOUNDARY_AABB = 0, MER_BOUNDARY_SPHERE = 1, MER_BOUNDARY_SDF = 2 };
enum { MER_PHASE_ISOTROPIC = 0, MER_PHASE_HG = 1 };
enum { MER_TR_WOODCOCK2 = 0, MER_TR_RATIO = 1 };
enum { MER_STRATEGY_BALANCE = 0, MER_STRATEGY_SINGLE = 1, MER_STRATEGY_MANUAL = 2, MER_STRATEGY_MAXIMUM = 3 /* MaxExpDist, src/medium/maxexp.h */ };
enum { MER_FILTER_BOX = 0, MER_FILTER_GAUSSIAN = 1 };
enum { MER_ALBEDO_CONST = 0, MER_ALBEDO_GRID = 1 };
/* device memory layout of an uploaded grid (the integer index contract stays (x,y,z)) */
/* device layouts of a 1-channel float32 grid (the index contract stays (x,y,z)): DENSE = the VOL payload; CELL8 = the 8 corners of every
   cell in one 32-byte record; BRICK27 = the 3x3x3 corners of every 2x2x2-cell brick in one 128-byte record (one cache line serves
   eight cells: half the memory requests of CELL8 along a ray).  CELL8 / BRICK27 are for the refractive-index field. */
enum { MER_LAYOUT_DENSE = 0, MER_LAYOUT_CELL8 = 1, MER_LAYOUT_BRICK27 = 2, MER_LAYOUT_BRICK125 = 3 /* 4x4x4-cell bricks: 5x5x5 corners per 512-byte record */,
       MER_LAYOUT_AUTO = 4 /* 1-channel float32 grids: BRICK27 up to 2^28 nodes (the records stay near the caches), CELL8 above (half the
                              bytes per fetch once every fetch goes to HBM; measured 256^3 .. 1024^3); other grids: DENSE */ };

/* replaces GridDataSource::loadFromFile header fields (src/volume/gridvolume.cpp:217-287) */
typedef struct {
    int32_t res[3];
    int32_t channels;               /* 1 or 3 */
    int32_t dtype;                  /* MER_VOL_F32 | MER_VOL_U8 */
    float   aabb_min[3], aabb_max[3];
    /* inverse of the plugin's `toWorld` (GridDataSource: m_worldToVolume = m_volumeToWorld.inverse(), src/volume/gridvolume.cpp:110,
       188-195), row-major 3x4; all zeros = identity.  worldToGrid = scale((res-1)/extents) * translate(-min) * world_to_volume. */
    float   world_to_volume[12];
} mer_grid_desc;

/* One entry of mer_scene_desc.emitters (Scene::getEmitters, src/librender/scene.cpp:854-898).  MER_EMITTER_POINT: emitter `point`
   (position, intensity -- as point_position / point_intensity); MER_EMITTER_AREA: emitter `area` on a `rectangle` (to_world, radiance --
   as area_to_world / area_radiance).  The fields of the other kind are ignored.  sampling_weight = the emitter's `samplingWeight`
   (src/librender/emitter.cpp:103; > 0, 1 in the XML by default): at every collision ONE emitter of each kind is sampled, emitter k with
   probability sampling_weight_k / (sum of the weights of its kind), and its sample is divided by that probability.
   MER_EMITTER_SPOT: emitter `spot` (src/emitters/spot.cpp:66-200), a point emitter with a cone -- list entries only.  to_world = its frame
   (row-major 3x4; the position is its translation column, `position` is ignored), intensity = its peak intensity, cutoff_angle_deg /
   beam_width_deg = `cutoffAngle` / `beamWidth` in degrees (0 <= beam <= cutoff <= 180; the XML defaults are 20 and 3/4 of the cutoff).  It
   joins the point emitters: same selection CDF, same connections, and every evaluation is multiplied by falloffCurve (:105-118) with
   cosTheta = z row of the inverse of to_world's linear part . (-d) -- not normalised, as the reference has it -- where d is the unit
   STRAIGHT-LINE direction from the shading point to the emitter, also for curved rays (the reference's volpath takes the emitter value from
   sampleDirect before the medium's curved eval, scene.cpp:854-874; heterogeneousrefractive.cpp:571-640).  The projection `texture` is not
   built.
   MER_EMITTER_ENVMAP: emitter `envmap` (src/emitters/envmap.cpp:100-645), an importance-sampled lat-long environment map -- list entries
   only, at most one ("The scene may only contain one environment emitter", src/librender/scene.cpp:512), and not together with a non-zero
   env_radiance.  envmap = a handle of mer_envmap_upload, env_scale = its `scale`, env_reserved = 0; to_world = its `toWorld` (row-major 3x4,
   the linear part a rotation within 1e-5, the translation ignored).  It takes the constant environment's place at every site: camera-ray
   and path escapes, the luminaire sample at each collision (its selection probability is 1: sampling_weight must be > 0 but does not
   scale it) and the phase-sampled look-up, with pdfDirect as the MIS partner.  Curved rays: DESIGN.md section 1.
   MER_EMITTER_AREA_DISK / MER_EMITTER_AREA_SPHERE: emitter `area` on a `disk` (src/shapes/disk.cpp:101-255) or a `sphere`
   (src/shapes/sphere.cpp:108-387) -- list entries only, with the fields of MER_EMITTER_AREA (to_world, radiance, sampling_weight).  The disk
   is the image of the unit disk in z = 0 under to_world, its normal to_world(Normal(0,0,1)); shear or a u / v scale that differs by more
   than 1e-3 is refused with the reference's messages; 1 / area = 1 / (pi |to_world e_x|^2).  The sphere has its centre at the translation
   column and the radius |to_world e_x|; its rotation is irrelevant, and a linear part that is not a uniform scale of a rotation (1e-3) is
   refused.  A linear part of negative determinant flips the normals (the reference's flipNormals; a rectangle's normal flips the same
   way): a flipped sphere emits inward.  Rectangles, disks and spheres are ONE kind: one selection CDF over their sampling weights in list
   order, two sampler numbers per sample, one-sided emission (area.cpp:104-109,158-183), all-absorbing occluders.  A sphere is sampled by
   Sphere::sampleDirect (the cone of directions from outside, uniformly by area from inside), so its pdfDirect depends on the reference
   point.  Every shape must be clear of the medium shape: an outward sphere apart from it (sphere boundary: centre distance > the sum of
   the radii; cube: distance from the centre to the box > radius); a flipped sphere apart from it or around it (centre distance + the
   boundary's radius < radius; cube: its farthest corner closer than the radius); a disk outside it (sphere boundary: the disk's point
   closest to the centre lies outside -- exact; cube: the disk's circumscribed square passes the rectangle / box test -- conservative: a
   disk near a cube's edge or corner can be refused although it does not touch).  Same scope as the rectangle: rif_mode = MER_RIF_CONST,
   index-matched cube / sphere boundary, no point or spot emitter outside the medium shape in the same list.
   MER_EMITTER_COLLIMATED: emitter `collimated` (src/emitters/collimated.cpp:56-134), a beam that is a delta in position and direction --
   list entries only, integrator = MER_INTEGRATOR_PTRACER only (no camera path can sample it: with volpath it is refused, it could only
   render black).  to_world = the beam's frame (row-major 3x4): the origin is its translation column, the direction the image of (0,0,1);
   a linear part that is not a rotation within 1e-4 is refused with the reference's message ("Scale factors in the emitter-to-world
   transformation are not allowed!", :63-65).  intensity = the beam's `power` (:61,85,123).  The other fields are ignored. */
#define MER_MAX_EMITTERS 32
enum { MER_EMITTER_POINT = 1, MER_EMITTER_AREA = 2, MER_EMITTER_SPOT = 3, MER_EMITTER_ENVMAP = 4, MER_EMITTER_AREA_DISK = 5, MER_EMITTER_AREA_SPHERE = 6,
       MER_EMITTER_COLLIMATED = 7 };
typedef struct {
    int32_t type;
    float   position[3], intensity[3];
    float   to_world[12];
    union {                                          /* a spot's angles overlay the radiance it does not have: the record keeps its size */
        float radiance[3];                           /* MER_EMITTER_AREA */
        struct { float cutoff_angle_deg, beam_width_deg, spot_reserved; };      /* MER_EMITTER_SPOT (spot_reserved: 0) */
        struct { mer_volume envmap; float env_scale, env_reserved; };           /* MER_EMITTER_ENVMAP (env_reserved: 0) */
    };
    float   sampling_weight;
} mer_emitter;

/* Flat scene: what Integrator::render() (include/mitsuba/render/integrator.h:74) sees through
   Scene/Sensor/Film/Medium/PhaseFunction/VolumeDataSource/Emitter objects. */
typedef struct {
    /* sensor `perspective` + film `hdrfilm` (src/sensors/perspective.cpp:130-158,247-269); the other sensor kinds: `sensor` below */
    int32_t width, height;
    float   fov_x_deg, near_clip, far_clip;
    float   cam_to_world[12];       /* row-major 3x4, columns (left,newUp,dir,origin): Transform::lookAt */
    int32_t rfilter; float rfilter_param;   /* box radius | gaussian stddev (src/rfilters) */
    /* integrator `volpath` (src/librender/integrator.cpp:190-225) */
    int32_t max_depth, rr_depth, hide_emitters;
    /* shape with `interior` medium, null BSDF (src/librender/shape.cpp:48-70) */
    int32_t boundary;
    float   bmin[3], bmax[3];
    float   sph_center[3], sph_radius;
    /* medium */
    int32_t sigma_mode;
    float   sigma_a[3], sigma_s[3]; /* homogeneous sigmaA / sigmaS */
    int32_t strategy, channel; float sampling_density, medium_sampling_weight;  /* homogeneous.cpp:156-228 */
    mer_volume density; float density_scale;     /* heterogeneous `density`, `scale` */
    int32_t albedo_mode; float albedo[3]; mer_volume albedo_grid;
    int32_t rif_mode; float rif_const; mer_volume rif;   /* heterogeneousrefractive `rif` */
    int32_t stepper; float stepsize;             /* `stepsize` (heterogeneousrefractive.cpp:208) */
    /* phase `hg` / `isotropic` */
    int32_t phase; float g;
    int32_t tr_estimator;
    /* emitter `constant` radiance; medium emission per unit density (config 5) */
    float   env_radiance[3];
    float   emission[3];
    /* emitter `point` (src/emitters/point.cpp): position + radiant intensity; all-zero intensity = none.  With curved rays the
       emitter is reached by mer_connect's shooting solver; an emitter outside the medium shape through the boundary
       (Snell refraction at the shape, exterior index 1: src/medium/heterogeneousrefractive.cpp:873-919,963-992). */
    float   point_position[3], point_intensity[3];
    /* film decomposition (src/librender/film.cpp:56-84): 0 = none, 1 = transient, 2 = bounce.  Transient: every radiance
       contribution is binned by its optical path length (sum of h*n along curved segments, length*n otherwise:
       src/integrators/bdpt/bdpt_proc.cpp:151-176,449-470) into frames = ceil((max_bound-min_bound)/bin_width) RGB slices.
       The film then is float[height][width][frames*3 + 2]: RGB per frame, alpha, weight (bdpt_proc.cpp:230-245,484-485).
       calibrated_transient != 0 leaves the camera edge out of the path length (bdpt_proc.cpp:163-170).
       Bounce: the same film, binned by the number of path edges instead -- every edge counts 1.0 where transient adds its optical
       length (bdpt_proc.cpp:179-187,335-381); no modulation. */
    int32_t decomposition; float min_bound, max_bound, bin_width; int32_t calibrated_transient;
    /* path-length modulation of a transient film (continuous-wave time of flight; PathLengthSampler,
       src/librender/pathlengthsampler.cpp:12-114): MER_MODULATION_*; lambda, phase in degrees, P, neighbors.  With a
       modulation the film has one frame and every contribution is weighted by correlationFunction(pathLength)
       (src/integrators/bdpt/bdpt_proc.cpp:446-447; src/librender/film.cpp:76-78). */
    int32_t modulation; float mod_lambda, mod_phase_deg; int32_t mod_P, mod_neighbors;
    /* BSDF of the medium's boundary shape: MER_BSDF_NULL (index-matched, src/librender/shape.cpp:48-70), MER_BSDF_HDIELECTRIC
       (src/bsdfs/hdielectric.cpp: smooth dielectric whose eta is the RIF at the hit point, exterior index 1) or
       MER_BSDF_HROUGHDIELECTRIC (its microfacet form: the rough_* fields at the end of this struct) */
    int32_t boundary_bsdf;
    /* boundary = MER_BOUNDARY_SDF: the medium shape is the negative region of this signed-distance grid (1-channel float32 volume,
       trilinear; the reference's `sdf` child of heterogeneousrefractive, src/medium/heterogeneousrefractive.cpp:366-375, negative
       inside :481).  Camera rays find it by sphere tracing, the dielectric normal is the normalized gradient (:980-984).
       mer_render only; the leaf entry points know the cube / sphere boundaries. */
    mer_volume sdf;
    /* `aggressivetracing` of heterogeneousrefractive (src/medium/heterogeneousrefractive.cpp:230,473-493,697-704): with the
       signed-distance boundary, a trace of length s first advances, WITHOUT inside tests, by min(depth below the surface -
       sdf_max_error, distance left) as long as that depth is at least Epsilon (1e-4), each such leg being int(d/h) full steps plus
       the remainder step, and walks what is left with the ordinary tested trace.  sdf_max_error = the volume's maxSDFError(). */
    int32_t aggressive_tracing;
    float   sdf_max_error;
    /* rif_mode = MER_RIF_ACOUSTIC: the ultrasound-modulated index of `acousticrifvolume` (src/volume/acousticrifvolume.cpp:101-106,
       224-342), evaluated analytically: n = n_o + n_max J_m(k_r r) cos(m phi), r = sqrt(y^2 + z^2), phi = atan2(y, z),
       k_r = 2 pi freq / speed; gradient and Hessian as written there (r clamped at 1e-8).  No `rif` volume. */
    float   ac_n_o, ac_n_max, ac_k_r;
    int32_t ac_mode;
    /* `method` of the heterogeneous medium (src/medium/heterogeneous.cpp:195-202): MER_METHOD_WOODCOCK (default) or MER_METHOD_SIMPSON --
       composite Simpson quadrature of the density along straight rays for the transmittance (integrateDensity, :301-376) and its
       inversion for the free flight (invertDensityIntegral, :419-544); sigma_mode = GRID, rif_mode = CONST only.  het_stepsize = the
       plugin's `stepSize`; 0 = inferred as the reference does (:245-257): 0.5 x the smallest voxel extent of the density / albedo grids. */
    int32_t method; float het_stepsize;
    /* emitter `area` on a `rectangle` shape (src/emitters/area.cpp:67-187, src/shapes/rectangle.cpp:99-222): the rectangle is the image of
       [-1,1]^2 x {0} under area_to_world (row-major 3x4, no shear: "Error: 'toWorld' transformation contains shear!"); one-sided -- radiance
       area_radiance into the half space of its normal toWorld(0,0,1) -- and all-absorbing otherwise (an emitter shape without a BSDF gets a
       diffuse one of reflectance 0, src/librender/shape.cpp:48-56): it shadows the environment.  Sampled at every real collision
       (Shape::sampleDirect, src/librender/shape.cpp:102-115: area sampling converted to solid angle) with the phase-function sample as its
       MIS partner (volpath.cpp:120-173,370-428).  All-zero radiance = none.  The rectangle lies outside the medium shape.  Straight rays
       (rif_mode = MER_RIF_CONST), index-matched cube / sphere boundary. */
    float   area_to_world[12], area_radiance[3];
    /* the integrator: MER_INTEGRATOR_VOLPATH (0: path tracing from the sensor, everything above) or MER_INTEGRATOR_PTRACER -- light tracing,
       the reference's `ptracer` (src/integrators/ptracer/ptracer_proc.cpp, src/librender/particleproc.cpp:107-270) and the t = 1 strategy of its
       `bdpt`: paths start at an emitter, every scattering vertex is connected to the sensor and splatted onto the pixel the connection
       arrives at.  It is the estimator for sources no camera path can sample (MER_EMITTER_COLLIMATED).  One light path per (pixel, sample
       index) of the shard, its sampler stream keyed by that pair as a camera path's is; a tile shard selects paths by pixel id, splats land
       anywhere on the film.  Film: the layout of mer_film_channels; a contribution goes into RGB with the reconstruction filter's table
       weights (ImageBlock::put); every (pixel, sample index) adds exactly 1 to that pixel's alpha and weight, so that after S samples
       weight = S everywhere and RGB / weight is the reference's setBitmap(accum, W H / particles) (ptracer_proc.cpp:200-204).  Straight rays:
       value = throughput x power x importance / dist^2 x phase x transmittance (PerspectiveCamera::sampleDirect), pixel = its uv.  Curved
       rays: the vertex is joined to the sensor by the shooting solver of mer_connect; value = sampleDirect's straight-line value x the
       curved connection's transmittance x the solver weight x phase at the launch direction, and the PIXEL COMES FROM THE ARRIVAL DIRECTION
       (getSamplePosition of mer_connect's revDir; src/libbidir/vertex.cpp:1334-1348, bdpt_proc.cpp:396-399,432); a failed connection or one
       outside the frame contributes nothing.  A decomposed film bins by the summed edge lengths (optical on curved segments) plus the
       connection edge plus the camera edge (the part outside the medium shape; left out under calibrated_transient).  max_depth / rr_depth as
       particleproc.cpp:163,258-267 (no eta^2 in the roulette) and ptracer_proc.cpp:171-176; the null boundary costs one depth, as in volpath.
       The null crossing of a connection counts against max_depth with straight rays (scene.cpp:619-678, as volpath's straight kernels have
       it); with curved rays a path is charged one null crossing at most, as volpath's curved kernels charge it (their emitter connection is
       free): ptracer and volpath hold the same scattering orders at every max_depth.
       Scope: the perspective sensor with a rigid cam_to_world (rotation within 1e-4); list entries of kind point, spot (toWorld without
       scale) and collimated; a cube or sphere with the null BSDF; homogeneous or gridded sigma_t, constant or gridded albedo; rif_mode CONST,
       TRILINEAR in the dense layout, BSPLINE3, ACOUSTIC; both steppers; steady, transient, bounce and modulated films.  NOT built, refused
       with a message before anything reaches the device: emission events (ptracer_proc.cpp:83-107) -- a point or spot emitter is not visible
       directly, exactly as in volpath --, a non-zero env_radiance, envmap and area entries, the legacy point_* / area_* fields, medium
       emission, the lens and orthographic sensors, the signed-distance boundary, dielectric boundaries, the CELL8 / BRICK record layouts of
       the index field, method = simpson, and mer_render_paths.  integrator_reserved = 0.  All zero = volpath.  Two words in front
       of the list pointer, which stays 8-byte aligned: no padding, and the sensor and rough_* fields keep their places at the end. */
    int32_t integrator, integrator_reserved;
    /* several emitters: n_emitters entries (at most MER_MAX_EMITTERS) of a HOST array the caller owns for the duration of the call (placed
       before the rough_* fields, which stay the last 12 bytes of the struct, pointer first: no padding); every call that takes the scene reads it (each context of a mer_multi uploads it in its own mer_render).  n_emitters = 0: the point_* and
       area_* fields above describe the (at most one) point and area emitter.  n_emitters > 0: those fields must be zero and the list holds
       every point and area emitter (the constant environment stays env_radiance).  Each entry is checked as the single emitter of its kind
       is; in addition every rectangle must lie outside the medium shape by an exact test (sphere: its closest point; cube: a rectangle /
       box overlap test), and a list with a rectangle must not hold a point emitter outside the shape (point samples are not tested
       against rectangles).  Rectangles are all-absorbing occluders: the nearest one ends a camera ray, look-up or escaping path; any one
       blocks the environment's luminaire sample; an area sample on rectangle k is blocked by every other rectangle in front of it. */
    const mer_emitter *emitters; int32_t n_emitters;
    /* the sensor (src/sensors/): MER_SENSOR_PERSPECTIVE (0, the pinhole above), MER_SENSOR_ORTHOGRAPHIC (orthographic.cpp:107-155: parallel
       rays, o = T (nearP.x, nearP.y, 0), d = normalize(T (0,0,1)), nearP = (1 - 2 sx, (1 - 2 sy) / aspect); mint = near_clip, maxt = far_clip,
       not rescaled, as the reference has it), MER_SENSOR_THINLENS (thinlens.cpp:293-322: the pinhole with an aperture of world-space radius
       aperture_radius focused at focus_distance) or MER_SENSOR_TELECENTRIC (telecentric.cpp:140-222: the orthographic view with an aperture
       of radius aperture_radius / |T e_x| focused at focus_distance / |T e_z|).  T = cam_to_world; fov_x_deg is read by the two
       perspective kinds only, and for the two parallel kinds the extent of the view is T's scale: cam_to_world may carry a non-uniform
       scale for them; it must be invertible for every kind but the pinhole, which is not checked.  The two lens
       kinds draw their aperture sample (nextSample2D, mapped by squareToUniformDiskConcentric) directly after the pixel sample
       (src/librender/integrator.cpp:147-179, ENeedsApertureSample); the other two draw nothing more.  aperture_radius >= 0 (the XML
       front end turns a thin lens's 0 into Epsilon as the reference does; here 0 is the pinhole's / orthographic ray on two more draws)
       and focus_distance > 0 for the lens kinds; both are ignored otherwise.  sensor_reserved = 0.  All zero = the pinhole.  Placed before the rough_* fields: no padding. */
    int32_t sensor; float aperture_radius, focus_distance; int32_t sensor_reserved;
    /* boundary_bsdf = MER_BSDF_HROUGHDIELECTRIC (src/bsdfs/hroughdielectric.cpp: microfacet dielectric whose eta is the RIF at the hit point,
       exterior index 1, eta taken as for hdielectric): MER_MICROFACET_* distribution, one isotropic roughness alpha (the XML default is 0.1;
       clamped to >= 1e-4 as src/bsdfs/microfacet.h:131-136), and visible-normal sampling (Heitz & d'Eon 2014) or the full distribution with
       Walter's alpha scaling 1.2 - 0.2 sqrt|cos theta_i| (0; always 0 for phong).  The surface vertex samples a point emitter that lies
       outside the medium shape (volpath.cpp:230-262); interior vertices then do no emitter sampling toward it.  Refused: a point emitter inside the
       shape, the area emitter.  All zero (with another boundary_bsdf): ignored. */
    int32_t rough_distribution; float rough_alpha; int32_t rough_sample_visible;
} mer_scene_desc;
enum { MER_METHOD_WOODCOCK = 0, MER_METHOD_SIMPSON = 1 };
enum { MER_SENSOR_PERSPECTIVE = 0, MER_SENSOR_ORTHOGRAPHIC = 1, MER_SENSOR_THINLENS = 2, MER_SENSOR_TELECENTRIC = 3 };
enum { MER_INTEGRATOR_VOLPATH = 0, MER_INTEGRATOR_PTRACER = 1 };
enum { MER_BSDF_NULL = 0, MER_BSDF_HDIELECTRIC = 1, MER_BSDF_HROUGHDIELECTRIC = 2 };
enum { MER_MICROFACET_BECKMANN = 0, MER_MICROFACET_GGX = 1, MER_MICROFACET_PHONG = 2 };   /* MicrofacetDistribution::EType order (microfacet.h) */
enum { MER_MODULATION_NONE = 0, MER_MODULATION_SINE, MER_MODULATION_SQUARE, MER_MODULATION_HAMILTONIAN, MER_MODULATION_MSEQ,
       MER_MODULATION_DEPTHSELECTIVE };
enum { MER_DECOMPOSITION_NONE = 0, MER_DECOMPOSITION_TRANSIENT = 1, MER_DECOMPOSITION_BOUNCE = 2 };

/* which part of the image-sample space this call renders (multi-GPU sharding):
   sample indices spp_begin + k*spp_stride, k in [0, spp_count); 32x32 image tiles t with
   t % tile_count == tile_rank. */
typedef struct {
    int32_t spp_begin, spp_count, spp_stride;
    int32_t tile_rank, tile_count;
} mer_shard;

/* a fluence grid (mer_fluence_create): res[a] cells on axis a over the box bmin ... bmax; cell (i, j, k) holds the points whose
   floor((p - bmin) / (bmax - bmin) * res) is (i, j, k) per axis: the cells are half-open, a point on bmax lies outside */
typedef int32_t mer_fluence;                                  /* handle, > 0 */
typedef struct { int32_t res[3]; float bmin[3], bmax[3]; } mer_fluence_desc;
/* a time-resolved fluence grid (mer_fluence_time_create): the same box, and `frames` bins of width t_bin from t_min on in optical path
   length; frame f holds the deposits with floorf((l - t_min) / t_bin) == f (half-open).  reserved must be 0. */
typedef struct { int32_t res[3]; float bmin[3], bmax[3]; int32_t frames; float t_min, t_bin; int32_t reserved; } mer_fluence_time_desc;
/* an exitance map (mer_exitance_create): res[0] x res[1] (u x v) cells on every face of the medium shape's boundary -- 6 faces for
   MER_BOUNDARY_AABB, 1 for MER_BOUNDARY_SPHERE -- and `frames` bins of width t_bin from t_min on in optical path length.  A steady map has
   frames == 1 and t_bin == 0.  cos_min: the acceptance cone about the outward normal (0 accepts every exit).  reserved must be 0. */
typedef int32_t mer_exitance;                                 /* handle, > 0, from the context's handle counter */
typedef struct { int32_t boundary; int32_t res[2]; int32_t frames; float t_min, t_bin, cos_min; int32_t reserved; } mer_exitance_desc;
/* the frequency-domain recorders (mer_fluence_fd_create, mer_exitance_fd_create): the box of a fluence grid or the raster and cone of an
   exitance map, and n_freq (1 ... MER_MAX_FREQUENCIES) wavenumbers k >= 0 in radians per unit of optical path length -- k = 2 pi f / c0 for
   the modulation frequency f and the vacuum speed of light c0 in scene units per second; k = 0 is the steady state.  The entries of
   wavenumber past n_freq and every reserved word must be 0.  Both structs are laid out without implicit padding (48 and 24 bytes before
   wavenumber). */
#define MER_MAX_FREQUENCIES 8
typedef struct { int32_t res[3]; float bmin[3], bmax[3]; int32_t n_freq; int32_t reserved[2]; double wavenumber[MER_MAX_FREQUENCIES]; } mer_fluence_fd_desc;
typedef struct { int32_t boundary; int32_t res[2]; float cos_min; int32_t n_freq; int32_t reserved; double wavenumber[MER_MAX_FREQUENCIES]; } mer_exitance_fd_desc;
/* a detector on the boundary of the medium shape (mer_sensitivity_create): the raster of an exitance map of res[0] x res[1] (u x v) cells per
   face, one `face` of it (0 ... 5 for MER_BOUNDARY_AABB, 0 for MER_BOUNDARY_SPHERE) and on that face the half-open cell window
   iu0 <= iu < iu1, iv0 <= iv < iv1; the acceptance cone cos_min about the outward normal (0 accepts every exit); the gate (t_min, t_bin) in
   optical path length (t_bin == 0: no gate).  reserved must be 0. */
typedef struct { int32_t boundary, res[2], face, iu0, iu1, iv0, iv1; float cos_min, t_min, t_bin; int32_t reserved; } mer_detector_desc;
/* a sensitivity grid (mer_sensitivity_create): the voxel grid of a fluence grid (res, bmin, bmax: half-open cells) and the detector */
typedef int32_t mer_sensitivity;                              /* handle, > 0, from the context's handle counter */
typedef struct { int32_t res[3]; float bmin[3], bmax[3]; mer_detector_desc det; } mer_sensitivity_desc;
/* an array of detectors and gates over one window (mer_sensitivity_array_create) */
typedef struct {
    int32_t res[3]; float bmin[3], bmax[3];
    mer_detector_desc det;     /* raster, face, window, cone, t_min, t_bin: as for mer_sensitivity_create */
    int32_t bin_u, bin_v;      /* one detector = bin_u x bin_v raster cells of the window */
    int32_t gates;             /* >= 1; gate g takes floorf((l - t_min) / t_bin) == g */
    int32_t scatter;           /* 0 | 1: also record the scattering grid K */
    int32_t reserved[2];       /* 0 */
} mer_sensitivity_array_desc;

enum {
    MER_C_PATHS = 0, MER_C_STEPS, MER_C_RIF_EVALS, MER_C_TENTATIVE, MER_C_REAL,
    MER_C_SEGMENTS, MER_C_NEE, MER_C_LOOP_ITERS, MER_C_ACTIVE_LANES,
    MER_C_CONNECT_UNITS,        /* solver units (traced rays) K_connect ran: a connection costs 3 ... 100+ */
    MER_C_CONNECT_STEPS,        /* sensitivity / Verlet steps inside them */
    MER_C_CONNECT_LANE_SLOTS,   /* 64 x the steps of the longest unit of every K_connect wave: CONNECT_STEPS / this = its active-lane fraction */
    MER_C_SIDE_SPAWNED,         /* luminaire-sample / look-up walks handed to a side-walk slot (option spawn_walks) */
    MER_C_SIDE_INLINE,          /* ... and those that ran in the path's own lane because the side-walk slot was still busy */
    MER_C_COUNT = 16
};

/* ---- context ------------------------------------------------------------------------------------ */
int  mer_abi_version(void);
/* replaces PluginManager::createObject + Scheduler worker setup (src/libcore/plugin.cpp:180-196) */
int  mer_context_create(int32_t device_id, mer_context **out);
void mer_context_destroy(mer_context *ctx);
const char *mer_last_error(mer_context *ctx);       /* ctx may be NULL: error of a failed create */
/* run kernels on this hipStream_t (NULL = default stream).  mer_render cuts its shard into a few independent pipelines: the first runs on
   this stream, the others on internal non-blocking streams that start after the work already queued on this stream (an event) and
   are joined into it before mer_render returns -- the caller sees one stream. */
int  mer_context_set_stream(mer_context *ctx, void *hip_stream);
int  mer_device_info(mer_context *ctx, char *name, int32_t name_len, int32_t *cu_count, int64_t *hbm_bytes);
/* Scheduling / A-B options of a context -- the analogue of the reference's Scheduler / RenderJob settings (block size, worker count:
   src/mitsuba/mitsuba.cpp:80-81,281).  None changes a per-path result (tested); they are NOT read from the process environment by the
   render calls (one hook: MER_OPTIONS="name=value,..." gives initial values when a context is created).  Names:
     pipes          concurrent pipelines a render is cut into (1..4, default 4)
     nslots         path-state slots over all pipelines (0 = 4 x the resident lanes of the chip)
     ksteps         eikonal steps / tentative collisions per lane per K_march launch (default 128)
     mq_sort        march lists sorted by steps-to-boundary class: -1 by field size (default), 0 off, 1 on
     lds_bricks     1 = K_march keeps every lane's current BRICK27 record in LDS (BRICK27 fields below 4 GiB) instead of re-gathering cells
                    through L1 / L2 (default 0: measured slower)
     connect_launches  K_connect launches per pass: each runs one solver unit (one traced ray) per pending curved-ray connection (default 2)
     adaptive_k     pass length in the tail of a render: 0 fixed (default), 1 longer, 2 shorter
     inline_walks   1 = straight rays in a gridded sigma_t: K_event runs the walks itself instead of handing them to K_march (default), 0 = two kernels
     spawn_walks    1 = curved rays, steady-state film: the transmittance walks of luminaire samples and emitter look-ups run in side-walk slots while
                    the path goes on to its next scattering event (default); 0 = every walk in the path's own lane
     check_every    passes per batch of launches; the host reads the finished-slot count back once per batch, two batches in flight (default 4)
     grid_fit       1 = launch grids sized by what the work lists can still hold -- live path slots x records per path + side walks in flight at
                    the last read-back -- instead of by every record (default); 0 = full grids (A/B)
     march_sort     curved rays: the march list of every pass is also counting-sorted by position (cells of a 2^b x 2^b x 2^b grid over the RIF's
                    box in Morton order, b = 1 ... 4) and swept in XCD-contiguous chunks; 0 = off (default: measured -40 % L2 misses, no gain in time)
     march_sort_major  bin order of that sort: 0 = cell-major (default), 1 = exit-time-class-major
     tile_deal      1 = image-tile shards dealt on diagonals of the tile grid (default), 0 = plain row-major round robin (whole tile columns)
     small_render_slots  1 = a render with fewer than ~8 paths per slot runs on a quarter of the slots (default)
     pass_events    per-pass HIP events feeding mer_last_render_stats (default 1)
     buffer_loads   0 = read fields with global loads even below 4 GiB, i.e. run the kernels a >= 4 GiB field selects (default 1)
     gen_all        K_gen hands every camera sample to K_event (A/B, default 0)
     prefilter      K_prefilter form: 0 register windows (default), 1 one thread per line, 2 two kernels per axis, 3 strided x, 4 LDS x
     march_lds_kb   KiB of unused dynamic LDS requested per K_march block: an occupancy cap for A/B runs (33 -> 4 blocks per CU, 41 -> 3; default 0)
     verbose, debug_pixel */
int  mer_context_set_option(mer_context *ctx, const char *name, int64_t value);
int  mer_context_get_option(mer_context *ctx, const char *name, int64_t *value);
/* libmer_check.so (the same sources built with -DMER_BOUNDS_CHECK): every index a kernel forms into a device buffer is compared with
   the buffer's extent; out = {violations since the last call, kind, index, limit of the first}; *enabled = 0 in the product build
   (which compiles the checks away and always reports zeros).  No reference analogue (the reference relies on host sanitizers). */
int  mer_debug_bounds(mer_context *ctx, int32_t *enabled, uint64_t out[4]);

/* ---- volumes: replaces GridDataSource / SplineDataSource construction
        (src/volume/gridvolume.cpp:108-198, src/volume/splinevolume.cpp:204-317) ------------------------- */
int  mer_volume_upload(mer_context *ctx, const mer_grid_desc *desc, const void *host_data,
                       int32_t layout, mer_volume *out);
/* same, from a device-resident dense grid (generated on the GPU) */
int  mer_volume_upload_dev(mer_context *ctx, const mer_grid_desc *desc, const void *data_dev,
                           int32_t layout, mer_volume *out);
/* Signed-distance grid of a triangle mesh, built on the GPU: the `sdf` child of heterogeneousrefractive for a shape given as faces.  The
   reference reads such a grid but has no tool that makes one (its exact inside test, winding numbers over the mesh, is commented out:
   src/medium/heterogeneousrefractive.cpp:732-739).
   desc: the grid -- channels = 1, dtype = MER_VOL_F32, world_to_volume all zero; node (i, j, k) lies at
   aabb_min[a] + (float) i * ((aabb_max[a] - aabb_min[a]) / (float) (res[a] - 1)) per axis, x fastest (the VOL payload order).
   vertices: host, n_vertices x xyz; triangles: host, n_triangles x 3 vertex indices.
   Per node, in float32: distance = min over the triangles of the point-triangle distance (closest point by Voronoi regions, Ericson,
   Real-Time Collision Detection 5.1.5); winding number w = (1 / 4 pi) sum_t 2 atan2(a . (b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|)
   with a, b, c = the triangle's vertices minus the node (Van Oosterom-Strackee).  The node is inside iff |w| >= 0.5 -- a mesh whose
   orientation is inverted as a whole gives the same grid, an open mesh degrades gracefully -- and the grid holds -distance inside,
   +distance outside (the convention of mer_scene_desc.sdf).
   Every node is tested against every triangle; the triangles are processed max_triangles_per_launch at a time (0 = default, 4096), one
   kernel launch per chunk and per 2^24 nodes, so that no launch runs long.  Every node adds its triangles in index order: the result is
   bit-identical for every chunk size.
   Refused with a message (mer_last_error) before anything reaches the device: res[a] < 2; more than 2^31 nodes; a box that is empty or
   not finite; n_triangles outside [1, 2^22]; an index outside [0, n_vertices); a vertex that is not finite; max_triangles_per_launch < 0;
   a non-zero world_to_volume.  Triangles with a repeated index or an exactly zero cross product (b - a) x (c - a) are dropped; a mesh
   with none left is refused.
   layout: as for mer_volume_upload_dev, whose path the result takes (a BRICK layout stays refused for an sdf at render time).
   winding_host: NULL, or one float per node that receives w.  *out: an ordinary volume handle (mer_volume_destroy). */
int  mer_sdf_from_mesh(mer_context *ctx, const mer_grid_desc *desc, const float *vertices, int64_t n_vertices,
                       const int32_t *triangles, int64_t n_triangles, int32_t max_triangles_per_launch,
                       int32_t layout, float *winding_host, mer_volume *out);
/* the dense x-fastest float32 payload of a 1-channel float32 volume (res[0] * res[1] * res[2] floats), whatever its device layout;
   refused for 3-channel and uint8 volumes and for envmap handles */
int  mer_volume_download(mer_context *ctx, mer_volume v, float *data_host);
/* builds cubic-B-spline coefficients on the GPU (Spline<3>::build3d, include/mitsuba/core/basisspline.h:812-890) */
int  mer_volume_build_spline(mer_context *ctx, mer_volume v);
int  mer_volume_download_spline(mer_context *ctx, mer_volume v, float *coeff_host);
int  mer_volume_destroy(mer_context *ctx, mer_volume v);
/* emitter `envmap` (src/emitters/envmap.cpp:100-190, 260-320): rgb_host = float32 [height][width][3], the lat-long image as loaded (level 0,
   no resampling).  The texels are rounded to IEEE half (the reference's TMIPMap<Spectrum, SpectrumHalf>), and the sampling tables are
   built from the rounded texels on the host in the reference's order and precision: a conditional luminance CDF per row, the row weights
   sin((y + 0.5) pi / height), the marginal CDF and the normalisation.  Fails as configure() does on an all-black or non-finite map.  The
   handle is freed by mer_volume_destroy (it is no grid: no other volume call takes it). */
int  mer_envmap_upload(mer_context *ctx, int32_t width, int32_t height, const float *rgb_host, mer_volume *out);

/* ---- film (ImageBlock, include/mitsuba/render/imageblock.h:124-205): float[height][width][channels], channels = 5
        (R,G,B,alpha,weight) in steady state; mer_film_channels() for a scene with a transient decomposition; the *_n
        variants take the channel count ------ */
int  mer_film_channels(mer_context *ctx, const mer_scene_desc *scene, int32_t *channels);
int  mer_film_alloc_n(mer_context *ctx, int32_t width, int32_t height, int32_t channels, float **film_dev);
int  mer_film_zero_n(mer_context *ctx, float *film_dev, int32_t width, int32_t height, int32_t channels);
int  mer_film_download_n(mer_context *ctx, const float *film_dev, int32_t width, int32_t height, int32_t channels, float *film_host);
int  mer_film_alloc(mer_context *ctx, int32_t width, int32_t height, float **film_dev);
int  mer_film_zero(mer_context *ctx, float *film_dev, int32_t width, int32_t height);
int  mer_film_download(mer_context *ctx, const float *film_dev, int32_t width, int32_t height, float *film_host);
int  mer_film_free(mer_context *ctx, float *film_dev);

/* ---- the hot path: replaces SamplingIntegrator::render -> renderBlock -> Li -> ImageBlock::put
        (src/librender/integrator.cpp:95-188, src/integrators/path/volpath.cpp:84-343).
        Accumulates (R,G,B,alpha,weight) splats into film_dev.  Launches on the context stream; returns when the
        last wavefront pass has been issued and found no live path (it synchronises the stream internally).
        scene->integrator = MER_INTEGRATOR_PTRACER: the light tracer instead (CaptureParticleWorker, ptracer_proc.cpp:167-194), one
        lane per light path in launches of a fixed number of paths; mer_shard keeps its meaning. ---- */
int  mer_render(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard,
                uint64_t seed, float *film_dev);
int  mer_synchronize(mer_context *ctx);
/* HIP-event time of the last mer_render kernel in ms (synchronizes) */
int  mer_last_kernel_ms(mer_context *ctx, float *ms);
/* wavefront passes of the last mer_render and the summed HIP-event device time of its K_march / K_event launches (summed over the
   concurrent pipelines: the sums can exceed the wall time) */
int  mer_last_render_stats(mer_context *ctx, int32_t *passes, float *march_ms, float *event_ms);
int  mer_counters_read(mer_context *ctx, uint64_t out[MER_C_COUNT]);    /* StatsCounter analogue */
int  mer_counters_reset(mer_context *ctx);

/* ---- the fluence inside the medium as a voxel grid, recorded from light paths: replaces the `fluencemeter` sensor driven by `ptracer`
        (src/sensors/fluencemeter.cpp:40-41, "the average radiance passing through a specified position"), one grid of probes instead of one
        probe per render.
        The estimator.  A light path is exactly the one mer_render walks for the same scene, shard and seed under integrator = ptracer: the
        same work id and (pixel, sample) sampler key, emitter selection and emitted ray, entry into the shape (one depth paid for the null
        boundary), free flights, phase-function samples and roulette, and the same bounds on the scatterings and march units of a path.
        There is no sensor connection: the sensor fields only enumerate the paths, width x height x samples of them, and the film fields
        (decomposition, modulation, filter) are ignored.  max_depth means what it means in the light tracer's loop: with an emitter outside
        the shape, max_depth = 2 keeps the first collisions only (the ballistic fluence).
        Every real collision the loop reaches is a collision-estimator sample of the fluence.  With T the path's throughput BEFORE it is
        multiplied by the albedo, the deposit is  w = T * power * (transmittance / pdfSuccess)  per channel -- 1 / sigma_t for delta
        tracking in a gridded sigma_t, tau_c / pdf for the homogeneous strategies -- into the cell that holds the collision point.  No
        refRatioSq is applied: particles carry power, and the light tracer applies none either.  A point outside the box deposits nothing;
        its w is added to the `dropped` total.
        The grid holds raw float64 sums, double[nz][ny][nx][3], added with float64 atomics.  fluence = sums / (paths * cell volume), per
        unit of whatever the emitter's intensity / power is in; sigma_a * fluence is the absorbed power density.  Raw sums of disjoint
        shards add (several GPUs: one grid per context, added by the caller).
        totals[8], kept beside the grid: [0] paths started; [1..3] escaped weight; [4..6] dropped deposit weight; [7] paths ended by a
        budget, a failed start gate (B-spline field) or no forward progress.
        The escaped weight.  A path whose free flight reaches the boundary leaves with  T * power * (transmittance / pdfFailure)  per
        channel, the light tracer's weight of a failed flight (particleproc.cpp:190-196): 1 for a gridded sigma_t; in a homogeneous
        medium tau_c(d) / pdfFailure(d) at the distance d to the boundary, pdfFailure = medium_sampling_weight * P(sampled distance > d)
        + (1 - medium_sampling_weight).  The factor is exactly 1, and not evaluated, when the three sigma_t are equal,
        medium_sampling_weight == 1 and the strategy is not manual.  On a curved ray d is the arc length of the steps inside plus half of the
        step that left the shape (the flight fails where it passes the boundary, somewhere inside that step; the relative error left in
        the weight is of the order (difference of the sigma_t x stepsize)^2 / 24).  A path that starts a flight on the boundary heading out, or whose emitted ray
        misses the shape, leaves with T * power.  A transmittance that underflowed to 0 over a pdfFailure of 0 weighs 0.
        sum(sigma_a * sums) + sigma_a * dropped + escaped = paths * power per channel in expectation when max_depth = -1, for every
        strategy, channel-dependent coefficients and any medium_sampling_weight > 0.
        Scope: exactly the light tracer's -- the scene must pass mer_render's checks for integrator = MER_INTEGRATOR_PTRACER unchanged (point,
        spot and collimated list entries; cube or sphere with the null boundary; homogeneous or gridded sigma_t; constant or gridded albedo;
        rif_mode CONST, dense TRILINEAR, BSPLINE3 or ACOUSTIC; both steppers), and any other integrator is refused, before any launch.
        mer_fluence_create: res 1 ... 1024 per axis, at most 2^27 cells, bmin < bmax per axis, all finite; the grid starts zeroed.
        mer_render_fluence ACCUMULATES into the grid (mer_fluence_clear zeroes it and the totals), launches on the context stream in the light
        tracer's chunks and returns synchronised; mer_counters_read afterwards reports the walk as it does after mer_render.
        mer_fluence_read: sums may be NULL (totals only).  mer_context_destroy frees the grids still alive.
        A handle of mer_fluence_track_create (below) makes mer_render_fluence deposit along every free flight instead -- the track-length
        estimator, which also fills cells without extinction; it needs analog distance sampling and loses, on curved rays, the piece of
        path before the boundary that is shorter than one stepsize. ---- */
int  mer_fluence_create(mer_context *ctx, const mer_fluence_desc *desc, mer_fluence *out);
int  mer_fluence_clear(mer_context *ctx, mer_fluence f);
int  mer_fluence_destroy(mer_context *ctx, mer_fluence f);
int  mer_render_fluence(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, uint64_t seed, mer_fluence f);
int  mer_fluence_read(mer_context *ctx, mer_fluence f, double *sums /* [nz][ny][nx][3] or NULL */, double totals[8]);

/* ---- time-resolved fluence: the deposits of mer_render_fluence binned by the optical path length at which they happen.  A time-resolved
        grid is a second kind of mer_fluence handle: mer_fluence_clear, mer_fluence_destroy, mer_render_fluence and mer_context_destroy take
        either kind, and mer_render_fluence picks the kernel by the handle's kind (a steady-state handle renders exactly as before).
        The estimator.  The walk is the steady-state one, draw for draw: for one scene, shard and seed both kinds of handle meet the same
        collisions with the same w.  The path length l of a deposit is what the light tracer's path length holds at that collision under a
        TRANSIENT film: the exterior leg from an emitter outside the shape (index 1), plus per free flight the optical length
        integral n ds of a curved ray or t * rif_const of a straight one, accumulated in float32.  The window is the handle's own: the
        film fields (decomposition, min_bound, bin_width, calibrated_transient, modulation) stay ignored.
        frame = floorf((l - t_min) / t_bin).  w goes to sums[frame][cell] when the point lies in the box and 0 <= frame < frames.
        The grid holds raw float64 sums, double[frames][nz][ny][nx][3].  time-resolved fluence = sums / (paths * cell volume * t_bin),
        per unit of optical path length; divide the path length by c to get time.  Summed over a window that holds every deposit, sums
        equals the steady-state grid's.  Raw sums of disjoint shards add.
        totals[12]: [0..7] as mer_fluence_read has them -- [4..6] is the dropped weight of points outside the box, at any time;
        [8..10] the weight of deposits inside the box but outside the time window; [11] is 0.
        mer_fluence_time_create: the box checks of mer_fluence_create; frames 1 ... 4096 (the film's cap); t_min finite; t_bin finite and
        greater than 0; reserved == 0; cells * frames at most 2^27.  *out = 0 on failure.
        mer_fluence_read refuses a time-resolved handle and mer_fluence_time_read a steady-state one.  sums may be NULL (totals only). ---- */
int  mer_fluence_time_create(mer_context *ctx, const mer_fluence_time_desc *desc, mer_fluence *out);
int  mer_fluence_time_read(mer_context *ctx, mer_fluence f, double *sums /* [frames][nz][ny][nx][3] or NULL */, double totals[12]);

/* ---- track-length fluence: a third kind of mer_fluence handle, a steady-state grid with the layout and totals of mer_fluence_create
        (double[nz][ny][nx][3] raw sums, then 8 totals), filled by the track-length estimator the users of photon-migration codes know.
        mer_fluence_clear, mer_fluence_destroy, mer_fluence_read, mer_render_fluence and mer_context_destroy take it; mer_fluence_time_read
        refuses it as it refuses every steady-state grid.  mer_render_fluence picks the kernel by the handle's kind; the other two kinds
        render exactly as before.
        The estimator.  The walk is the collision grid's, draw for draw (the deposit draws no sampler number): for one scene, shard and
        seed the counters, totals[0] (paths), totals[1..3] (escaped) and totals[7] (ended) equal those of a mer_fluence_create handle.
        Instead of one deposit at the collision, every free flight deposits along the piece of path it flew inside the shape -- from the
        flight's start to the real collision or to the exit, the whole in-shape chord including any part outside the density grid's box --
        cut at the faces of the grid's (half-open) cells.  Cell c, crossed between the flight parameters a and b (arc length from the
        flight's start), receives per channel
            w_c = T_c * power_c * integral_a^b tau_c(s) / S(s) ds
        with T the throughput at the flight's start, tau_c the channel's transmittance and S(s) the probability that the sampled distance
        exceeds s.  This is unbiased for any distance sampling; it is BUILT for the analog cases, where S is one exponential exp(-rho s):
        a gridded sigma_t (delta tracking: rho = sigma(x), w = T * power * (b - a)), or a homogeneous sigma_t with medium_sampling_weight
        == 1 and strategy single or manual (rho = the sampling density) or balance with three equal sigma_t (rho = sigma_t).  With
        Delta_c = sigma_t,c - rho and l = b - a:  w_c = T_c power_c exp(-Delta_c a) (-expm1(-Delta_c l)) / Delta_c, and exactly
        T_c power_c l when Delta_c == 0.  Where sigma_t is 0 -- a clear cuvette, a void of a density grid, a clear gradient-index medium --
        the collision grid stays 0 and this one holds power x length.  No refRatioSq, as in the collision grid; max_depth keeps its meaning.
        The analog requirement.  mer_render_fluence refuses, before any launch and only for a track-length handle, a homogeneous medium
        with strategy balance and channel-dependent sigma_t, strategy maximum, or medium_sampling_weight != 1 after the default is
        resolved: their S is no single exponential.
        Curved rays.  Every eikonal step that passed the inside test deposits along its chord, split at the cell faces, at the arc length
        the walk has accumulated.  The step that left the shape and the step back after it deposit nothing: the last piece of path
        before the boundary, shorter than one stepsize, is lost, as it is for the walk itself.
        totals[8]: [0] paths; [1..3] escaped weight; [4..6] weight x length of the pieces outside the box; [7] ended.
        The escaped weight is mer_fluence_create's: with rho the sampling density, T_c power_c exp(-Delta_c d) at the distance d to
        the boundary.  sum(sigma_a * sums) + sigma_a * dropped + escaped = paths * power holds per channel in expectation, as stated for
        mer_fluence_create, not per path.  fluence = sums / (paths * cell volume), as for the collision grid.
        mer_fluence_track_create: the descriptor and the checks of mer_fluence_create, under its own message prefix. ---- */
int  mer_fluence_track_create(mer_context *ctx, const mer_fluence_desc *desc, mer_fluence *out);

/* ---- exitance maps: where and when light paths leave the medium.  Replaces a grid of `irradiancemeter` probes on the medium shape
        (src/sensors/irradiancemeter.cpp, driven by `ptracer`): one accumulator over the whole boundary instead of one probe per render.
        mer_exitance is its own kind of handle: the mer_fluence_* entry points refuse it as an unknown handle, and the entry points below
        refuse a fluence handle the same way.
        The walk.  A light path is exactly the one mer_render_fluence walks for the same scene, shard and seed: work id and sampler key,
        emitter selection and emitted ray, entry with one depth paid for the null boundary, free flights, phase-function samples, roulette
        and the bounds on the scatterings and march units of a path.  Recording an exit draws no sampler number, fetches no RIF value and
        advances no counter: mer_counters_read, totals[0] (paths), totals[1..3] (escaped) and totals[7] (ended) equal those of a
        mer_fluence_create render.
        The exit.  With the null boundary and a convex shape a path leaves at most once.  At that moment it records
          x, d   straight rays: x = the intersection of the last flight with the shape (the flight's start when the path stands on the
                 boundary heading out), d = the flight's direction.  Curved rays: from the walk's last point inside, x0, along
                 d = normalize(optical momentum), the shape is hit again (the re-hit of the dielectric boundary, after edge.cpp:45-60):
                 x = x0 + d t, or x0 when there is no hit.
          w      what `escaped` receives: T * power * (transmittance / pdfFailure) per channel for a flight that reached the boundary
                 (mer_fluence_create, the escaped weight), T * power for a path that starts a flight on the boundary heading out.
          l      the optical path length the time-resolved fluence grid carries (the exterior leg at index 1, then per free flight
                 integral n ds or t * rif_const, in float32) plus the last flight: its length times rif_const, or its integral n ds on a
                 curved ray.  The piece between x0 and x is not added: it is shorter than one stepsize, the loss the walk and the
                 track-length grid document.
        Acceptance.  c = dot(d, outward normal at x).  With cos_min > 0 an exit with c < cos_min is not binned: its w goes to `rejected`.
        The cone is measured at the surface in the medium's own index: the index-matched boundary does not refract.
        Window.  A timed map (t_bin > 0): frame = floorf((l - t_min) / t_bin); outside 0 <= frame < frames, w goes to `late`.  A steady
        map (frames == 1, t_bin == 0) puts everything into frame 0.
        Cell, cube (6 faces): the axis and sign of the face by the rule of the boundary normal (the axis on which |x - centre| / half
        size is largest, first axis on a tie; sign + when x >= centre); face = 2 * axis + (sign > 0); ua = (axis + 1) % 3,
        va = (axis + 2) % 3; iu = clamp(floor((x[ua] - bmin[ua]) / (bmax[ua] - bmin[ua]) * res_u), 0, res_u - 1), iv the same on va.
        Clamped, not dropped: the point is on the boundary by construction.
        Cell, sphere (1 face, equal-area cells): q = (x - c) / |x - c|; iv from (1 + q.z) / 2, iu from atan2(q.y, q.x) / 2 pi wrapped
        into [0, 1); both clamped.
        An emitted ray that misses the shape has no exit point: its weight goes to `missed`.
        The map holds raw float64 sums, double[frames][faces][res_v][res_u][3], at most 2^27 keys; raw sums of disjoint shards add (the
        caller reduces them).  exitance = sums / (paths * cell area [* t_bin for a timed map]).
        totals[16]: [0] paths; [1..3] escaped, as the fluence grids have it (the missed weight included); [4..6] missed; [7] ended;
        [8..10] late; [11..13] rejected; [14] the number of exits binned; [15] 0.  Every escaping path goes to exactly one of sums,
        missed, rejected (tested first) or late: sum(sums) + missed + rejected + late = escaped per channel, up to float64 summation
        order, for any medium and not only in expectation.
        mer_exitance_create refuses, each with its own message and *out = 0: a boundary that is neither kind; res outside 1 ... 4096;
        frames outside 1 ... 4096; t_bin negative or not finite, or t_bin == 0 with frames != 1; t_min not finite; cos_min outside
        0 <= cos_min < 1; reserved != 0; more than 2^27 keys.  The map starts zeroed.
        mer_render_exitance requires integrator = ptracer and the light tracer's scope unchanged, refuses a scene whose boundary differs
        from the map's, ACCUMULATES (mer_exitance_clear zeroes the map and the totals), launches in the light tracer's chunks on the context
        stream and returns synchronised.  mer_exitance_read: sums may be NULL (totals only).  mer_context_destroy frees the maps alive.
        Out of scope, refused by the light tracer's unchanged checks: dielectric and signed-distance boundaries, sensors other than
        perspective, area / envmap / constant emitters.  Also not built: several GPUs in one call, angular histograms beyond the one
        acceptance cone. ---- */
int  mer_exitance_create(mer_context *ctx, const mer_exitance_desc *desc, mer_exitance *out);
int  mer_exitance_clear(mer_context *ctx, mer_exitance e);
int  mer_exitance_destroy(mer_context *ctx, mer_exitance e);
int  mer_render_exitance(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, uint64_t seed, mer_exitance e);
int  mer_exitance_read(mer_context *ctx, mer_exitance e, double *sums /* [frames][faces][res_v][res_u][3] or NULL */, double totals[16]);

/* ---- frequency-domain fluence grids and exitance maps: the response to an intensity-modulated source, the third standard measurement of
        photon migration beside the steady state and the pulse.  The field at a point, and the signal at a detector, is a complex number
        whose modulus is the amplitude and whose argument is the phase lag of the photon-density wave.  A frequency-domain grid is a further
        kind of mer_fluence handle and a frequency-domain map a second kind of mer_exitance handle: mer_fluence_clear / mer_exitance_clear,
        mer_fluence_destroy / mer_exitance_destroy, mer_render_fluence / mer_render_exitance and mer_context_destroy take them, and the
        render entry points pick the kernel by the handle's kind (every other kind renders exactly as before).
        The estimator.  The walk is mer_render_fluence's / mer_render_exitance's, draw for draw: recording draws no sampler number, fetches
        no RIF value and advances no counter, so for one scene, shard and seed the counters, totals[0] and totals[7] equal those of the
        steady handles.  A handle holds n_freq wavenumbers k_j.
          grid   every real collision deposits into the cell of the collision point, per channel, with the weight w of mer_fluence_create
                 and the optical path length l that mer_fluence_time_create bins (float32: the exterior leg at index 1, then per free
                 flight integral n ds on a curved ray or t * rif_const on a straight one):  w cos(k_j l) into the real plane of frequency
                 j and w sin(k_j l) into its imaginary plane.
          map    the one exit of a path adds w (cos, sin)(k_j l) to the cell of x, with x, d, w and l exactly what mer_render_exitance
                 records (l includes the last flight).  cos_min applies as it does there; there is no window: `late` stays 0.
        Phase arithmetic.  phi = k_j * (double) l with k_j kept in float64; phi is reduced to [-pi, pi] in float64, rounded to float32
        once, and cos / sin are float32: each has an absolute error of at most 2^-21 (pi 2^-24 from the rounding, 2 ulp from the
        functions).  The pair is then scaled to unit modulus in float64 (to within 1e-12) and multiplied with w in float64, so that no
        deposit weighs more than its w.  k = 0 gives exactly (1, 0): its real plane receives the deposits of the steady handle, and its
        imaginary plane is never written and stays exactly 0.0.
        Layout.  Raw float64 sums, added with float64 atomics, plane (2 j + part) for part 0 = real, 1 = imaginary:
          grid   double[n_freq][2][nz][ny][nx][3]; complex fluence = sums / (paths * cell volume)
          map    double[n_freq][2][faces][res_v][res_u][3]; complex exitance = sums / (paths * cell area)
        at most 2^27 keys (cells x 2 x n_freq).  Raw sums of disjoint shards add.  amplitude = hypot(re, im), phase = atan2(im, re); the
        modulus never exceeds the steady sum of the same paths.
        Totals.  mer_fluence_fd_read: the 8 of mer_fluence_read, [4..6] the plain w of the points outside the box.  mer_exitance_fd_read:
        the 16 of mer_exitance_read; [8..10] (late) stay 0, [14] counts the exits binned once, not per plane.
        Refusals.  mer_fluence_fd_create: the box checks of mer_fluence_create; mer_exitance_fd_create: the boundary, res and cos_min
        checks of mer_exitance_create; both, each with its own message and *out = 0: n_freq outside 1 ... MER_MAX_FREQUENCIES; a wavenumber
        that is negative or not finite; a non-zero entry past n_freq; a non-zero reserved word; more than 2^27 keys.
        mer_fluence_read, mer_fluence_time_read and mer_exitance_read refuse a frequency-domain handle and name the reader to use;
        mer_fluence_fd_read and mer_exitance_fd_read refuse every other kind the same way.  sums may be NULL (totals only).
        Scope: exactly that of mer_render_fluence / mer_render_exitance.  Not built: a frequency-domain track-length grid,
        frequency-domain sensitivity grids, several GPUs in one call. ---- */
int  mer_fluence_fd_create(mer_context *ctx, const mer_fluence_fd_desc *desc, mer_fluence *out);
int  mer_fluence_fd_read(mer_context *ctx, mer_fluence f, double *sums /* [n_freq][2][nz][ny][nx][3] or NULL */, double totals[8]);
int  mer_exitance_fd_create(mer_context *ctx, const mer_exitance_fd_desc *desc, mer_exitance *out);
int  mer_exitance_fd_read(mer_context *ctx, mer_exitance e, double *sums /* [n_freq][2][faces][res_v][res_u][3] or NULL */, double totals[16]);

/* ---- sensitivity maps: which part of the medium did the light that reached a detector travel through.  The absorption sensitivity of
        the detected signal -- the Jacobian of diffuse optical tomography, the photon-measurement density function, the "banana" between
        a source and a detector, the mean partial path length per voxel -- by the method photon-migration codes call replay.  The
        reference has no analogue; the nearest is one `irradiancemeter` render per perturbed voxel.
        mer_sensitivity is its own kind of handle: the mer_fluence_* and mer_exitance_* entry points refuse it as an unknown handle, and
        the entry points below refuse theirs the same way.
        The walk.  A light path is exactly the one mer_render_exitance walks for the same scene, shard and seed, and its exit (x, d, w,
        l) is the one stated there.  totals[0] (paths), totals[7] (ended) and mer_counters_read equal mer_render_exitance's.
        The detector.  A path is DETECTED when its exit passes, in mer_render_exitance's own expressions: the cone (with cos_min > 0 an
        exit with dot(d, outward normal at x) < cos_min is rejected), then the gate (t_bin > 0: detected iff
        floorf((l - t_min) / t_bin) == 0), then the window (the exit's cell lies on `face` with iu0 <= iu < iu1 and iv0 <= iv < iv1).
        The detected weight totals[1..3] therefore equals the sum over the window's cells of a one-frame exitance map with the same
        raster, cone and gate, up to float64 summation order.
        The estimator.  A detected path leaves with weight w (RGB), known only at its exit, so every chunk of paths is walked twice: the
        first pass lists the detected paths with their w, the second re-walks exactly those -- the sampler stream is keyed by the work
        id -- and every free flight deposits w * length for the piece of the flight inside each cell of the grid:
            J_c = sum over the detected paths of w * L_c,      L_c = the length the path travelled inside cell c.
        The pieces are cut at the faces of the (half-open) cells exactly as the track-length fluence grid cuts them; the exterior leg of
        an emitter outside the shape deposits nothing.  Curved rays: every eikonal step that passed the inside test deposits along its
        chord; the step that left the shape and the step back after it deposit nothing, so the last piece of path before the boundary,
        shorter than one stepsize, is lost, as it is for the walk and for the track-length grid.
        Interpretation.  With S = W_det / paths the detected signal per emitted path, dS / d sigma_a(c) = -J_c / paths for a change of
        the absorption in cell c at fixed sigma_s.  This holds for every distance-sampling strategy -- only the integrand depends on
        sigma_a -- so unlike the track-length fluence grid there is NO analog requirement.  J_c / W_det is the mean partial path length in
        cell c of the detected light.
        The grid holds raw float64 sums, double[nz][ny][nx][3], at most 2^27 cells; raw sums of disjoint shards add (the caller reduces).
        totals[16]: [0] paths; [1..3] the detected weight W_det; [4..6] dropped: w * the length of the pieces outside the box; [7] ended
        (first pass); [8] the number of detected paths; [9..11] sum over the detected paths of w * the path's length inside the shape,
        summed per path in float64 from the flight lengths, before any cutting (straight rays: the distance to the collision or to the
        boundary; curved rays: the length of every step that deposited): sum(sums) + dropped = [9..11] per channel up to the float32
        arithmetic of the pieces; [12] replay disagreements: the paths whose second walk did not leave with the bits of the recorded w
        -- 0 unless the two passes walked different paths; [13..15] 0.
        mer_sensitivity_create refuses, each with its own message and *out = 0: the box checks of mer_fluence_create; the boundary, res,
        t_bin, t_min, cos_min and reserved checks of mer_exitance_create; a face outside the boundary's faces; a window that is empty or
        leaves the raster.  The grid starts zeroed.
        mer_render_sensitivity requires integrator = ptracer and the light tracer's scope unchanged, refuses a scene whose boundary
        differs from the detector's, ACCUMULATES (mer_sensitivity_clear zeroes the grid and the totals) and returns synchronised.  Per
        chunk of the light tracer's launches it reads the number of detected paths back and launches the second pass over exactly that
        many (none when it is 0); the list of one chunk's paths lives in the context and is freed with it.  mer_sensitivity_read: sums
        may be NULL (totals only).  mer_context_destroy frees the grids alive.
        Detector arrays, gates and the scattering grid (mer_sensitivity_array_create).  A time-domain measurement is one source, a raster
        of detectors and a row of gates; a path leaves through one raster cell at one path length, so it belongs to at most one
        measurement and the two passes fill every grid at once.  One detector is bin_u x bin_v raster cells of the window: ndu =
        (iu1 - iu0) / bin_u, ndv = (iv1 - iv0) / bin_v; gate g takes the exits with floorf((l - t_min) / t_bin) == g, 0 <= g < gates
        (gates == 1 and t_bin == 0: no gate); cone, gate expression and raster cell are those above.  An exit in raster cell (iu, iv)
        and gate g is measurement m = (g * ndv + (iv - iv0) / bin_v) * ndu + (iu - iu0) / bin_u of M = gates * ndv * ndu.  The handle is a
        mer_sensitivity: mer_render_sensitivity, _clear and _destroy take it as they are; mer_sensitivity_create(desc) means bin = the
        whole window, gates = 1, scatter = 0.
            J[m]  the absorption grid of measurement m, as above, over the paths of m (key m * n_cells + cell).
            K[m]  scatter = 1: the scattering grid (key (M + m) * n_cells + cell): every real collision a detected path scatters from
                  deposits the path's weight at the detector, w, into the cell that holds the collision point (mer_render_fluence's
                  cell): K_c = sum over the detected paths of w * N_c, N_c = the path's scattering collisions in cell c.
        In all (1 + scatter) * M * n_cells <= 2^27 keys.
        mer_sensitivity_read_array: sums double[1 + scatter][gates][ndv][ndu][nz][ny][nx][3] (or NULL), meas double[gates][ndv][ndu][8]
        (or NULL) and the totals.  meas[m]: [0..2] the detected weight of m, [3] its detected paths (first pass); [4..6] the sum over
        its paths of w * the path's number of scattering collisions, counted before any box test (second pass; 0 when scatter = 0);
        [7] 0.  totals[0..12] keep their meaning, summed over all measurements; totals[13..15]: scatter = 1: w per collision outside
        the box, so that sum(K) + totals[13..15] = sum over m of meas[m][4..6] per channel; 0 otherwise.  mer_sensitivity_shape: gates,
        ndv, ndu, scatter.  Both take handles made either way; mer_sensitivity_read refuses, by name, a handle with M > 1 or scatter = 1.
        Interpretation of K.  In a medium with homogeneous sigma_s, per channel and for every distance-sampling strategy, with S_m the
        detected signal of measurement m per emitted path: dS_m / d sigma_s = (sum(K[m]) / sigma_s - sum(J[m])) / paths, and per cell
        dS_m / d sigma_s(c) = (K_c / sigma_s - J_c) / paths.  The reason: a path's contribution carries one factor sigma_s per
        scattering vertex and exp(-sigma_s L) along its length, and the sampling density is held fixed.  With a gridded sigma_t or
        albedo K is delivered raw (w per collision) and its interpretation is left to the caller.
        mer_sensitivity_array_create refuses, each with its own message under its own prefix and *out = 0: everything
        mer_sensitivity_create refuses, in the same words; bin_u or bin_v < 1 or not dividing the window; gates < 1; gates > 1 with
        t_bin == 0; scatter other than 0 or 1; reserved != 0; more than 2^27 keys.
        Not built: sensitivities to the index field, several GPUs in one call. ---- */
int  mer_sensitivity_create(mer_context *ctx, const mer_sensitivity_desc *desc, mer_sensitivity *out);
int  mer_sensitivity_array_create(mer_context *ctx, const mer_sensitivity_array_desc *desc, mer_sensitivity *out);
int  mer_sensitivity_shape(mer_context *ctx, mer_sensitivity s, int32_t shape[4] /* gates, ndv, ndu, scatter */);
int  mer_sensitivity_read_array(mer_context *ctx, mer_sensitivity s,
                                double *sums /* [1 + scatter][gates][ndv][ndu][nz][ny][nx][3] or NULL */,
                                double *meas /* [gates][ndv][ndu][8] or NULL */, double totals[16]);
int  mer_sensitivity_clear(mer_context *ctx, mer_sensitivity s);
int  mer_sensitivity_destroy(mer_context *ctx, mer_sensitivity s);
int  mer_render_sensitivity(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, uint64_t seed, mer_sensitivity s);
int  mer_sensitivity_read(mer_context *ctx, mer_sensitivity s, double *sums /* [nz][ny][nx][3] or NULL */, double totals[16]);

/* ---- leaf entry points for parity tests (host pointers, batched SoA) ------------------------------ */
/* GridDataSource::lookupFloat (gridvolume.cpp:337-388); out_idx[4*i..] = x1,y1,z1,linear index or -1 */
int  mer_lookup_trilinear(mer_context *ctx, mer_volume v, const float *pts, int64_t n, float *out_val, int32_t *out_idx);
/* GridDataSource::lookupSpectrum (gridvolume.cpp:390-421) */
int  mer_lookup_trilinear_rgb(mer_context *ctx, mer_volume v, const float *pts, int64_t n, float *out_rgb);
/* VolumeDataSource::valueAndGradient (splinevolume.cpp:354-360) for rif_interp in {TRILINEAR,BSPLINE3} */
int  mer_rif_value_grad(mer_context *ctx, mer_volume v, int32_t rif_interp, const float *pts, int64_t n,
                        float *out_val, float *out_grad);
/* AcousticRIFVolume::valueAndGradient (acousticrifvolume.cpp:224-342) of the scene's analytic field (rif_mode = acoustic) */
int  mer_acoustic_value_grad(mer_context *ctx, const mer_scene_desc *scene, const float *pts, int64_t n,
                             float *out_val, float *out_grad);
/* HeterogeneousRefractiveMedium::trace / traceTillBoundary (heterogeneousrefractive.cpp:671-691,742-776);
   dist[i] = +inf selects traceTillBoundary */
int  mer_er_trace(mer_context *ctx, const mer_scene_desc *scene, const float *p0, const float *d0, const float *dist,
                  int64_t n, float *out_p, float *out_v, float *out_dist_surf, float *out_opt, int32_t *out_success);
/* Medium::sampleDistance (heterogeneous.cpp:589-663, homogeneous.cpp:275-352, heterogeneousrefractive.cpp:402-568);
   rec stride 20: success,t,p[3],sigmaS[3],transmittance[3],pdfSuccess,pdfFailure,refRatioSq,d[3],0,0,0;
   RNG stream of item i = (seed, pixel=i, sample=0) */
int  mer_sample_distance(mer_context *ctx, const mer_scene_desc *scene, const float *o, const float *d,
                         const float *maxt, int64_t n, uint64_t seed, float *rec);
/* Medium::evalTransmittance (heterogeneous.cpp:546-587 / ratio tracking) */
int  mer_eval_transmittance(mer_context *ctx, const mer_scene_desc *scene, const float *o, const float *d,
                            const float *maxt, int64_t n, uint64_t seed, float *out_tr);
/* HeterogeneousRefractiveMedium::eval -> makeDirectConnections (heterogeneousrefractive.cpp:571-640,798-1163): connect p1 to p2
   (p1 inside the medium shape -- cube, sphere or signed-distance grid --, p2 inside or outside it) by a curved ray; out stride 12: ok, weight, dirToP2[3] (optical momentum at p1),
   revDirToP1[3], distance, opticalLength, 0, 0; RNG stream of item i = (seed, pixel=i, sample=0) */
int  mer_connect(mer_context *ctx, const mer_scene_desc *scene, const float *p1, const float *p2, int64_t n, uint64_t seed, float *out);
/* PointEmitter / SpotEmitter::sampleDirect (src/emitters/point.cpp, spot.cpp:184-199) of entry k of the scene's emitter list (a point or a
   spot) at n reference points ref[3*i..]: out stride 8: value RGB (intensity x falloff / dist^2, NOT divided by the selection pdf), the unit
   direction to the emitter [3], the distance, the falloff (1 for a point).  The render kernels' own device function. */
int  mer_emitter_direct(mer_context *ctx, const mer_scene_desc *scene, int32_t k, const float *ref, int64_t n, float *out);
/* AreaLight::sampleDirect (src/emitters/area.cpp:158-173) through Shape / Sphere::sampleDirect (shape.cpp:102-115, sphere.cpp:286-355) of
   entry k of the scene's emitter list (an area emitter on a rectangle, disk or sphere) at n reference points ref[3*i..] with the samples
   u2[2*i..]: out stride 12: radiance / pdf RGB (NOT divided by the selection pdf; 0 from the back side), the unit direction d[3], the
   distance, the solid-angle pdf (0 from the back side), the normal n[3] at the sampled point, 0.  The render kernels' own device function. */
int  mer_area_direct(mer_context *ctx, const mer_scene_desc *scene, int32_t k, const float *ref, const float *u2, int64_t n, float *out);
/* Scene::rayIntersect restricted to the area emitters' shapes, then AreaLight::eval and pdfDirect (area.cpp:104-109,175-183): the nearest
   rectangle, disk or sphere along o[3*i..] + t d[3*i..], t >= 0 (d need not be unit: t is in its units); out stride 8: the entry's index in
   the emitter list or -1, t, the radiance seen along d RGB (0 from the back side), pdfDirect of the hit point from the reference point
   ref[3*i..] in the solid-angle measure (without the selection pdf), 0, 0.  The render kernels' own device functions. */
int  mer_area_hit(mer_context *ctx, const mer_scene_desc *scene, const float *o, const float *d, const float *ref, int64_t n, float *out);
/* EnvironmentMap::evalEnvironment (level 0, bilinear) and pdfDirect (envmap.cpp:385-415, 531-645) of the scene's envmap entry for n world
   directions dirs[3*i..] (need not be unit): out_rgb[3*i..] = value x scale, out_pdf[i] = the solid-angle density of the luminaire
   sample.  The render kernels' own device functions. */
int  mer_envmap_eval(mer_context *ctx, const mer_scene_desc *scene, const float *dirs, int64_t n, float *out_rgb, float *out_pdf);
/* EnvironmentMap::sampleDirect (envmap.cpp:516-610) for n samples u2[2*i..]: out_dir[3*i..] = the world direction, out_value_over_pdf[3*i..]
   = value x scale / pdf (0 when pdf is 0), out_pdf[i] = pdf.  The render kernels' own device function. */
int  mer_envmap_sample(mer_context *ctx, const mer_scene_desc *scene, const float *u2, int64_t n, float *out_dir, float *out_value_over_pdf,
                       float *out_pdf);
/* PhaseFunction::sample / eval (src/phase/hg.cpp:74-110, src/phase/isotropic.cpp:62-78) */
int  mer_phase_sample(mer_context *ctx, int32_t phase, float g, const float *wi, const float *u2, int64_t n, float *wo, float *pdf);
int  mer_phase_eval(mer_context *ctx, int32_t phase, float g, const float *wi, const float *wo, int64_t n, float *val);
/* RoughDielectric::eval / pdf and sample (src/bsdfs/hroughdielectric.cpp:131-289,383-507) of the scene's rough_* parameters, ERadiance, for
   per-item eta (interior / exterior index).  Vectors in the local shading frame (z = the outward normal), wi pointing away from the surface.
   out_val = f |cos theta_o|.  sample: u3[3*i..] = the microfacet sample (2D) and the reflect / refract choice; weight = eval / pdf (0: no sample) */
int  mer_rough_dielectric_eval(mer_context *ctx, const mer_scene_desc *scene, const float *eta, const float *wi, const float *wo, int64_t n,
                               float *out_val, float *out_pdf);
int  mer_rough_dielectric_sample(mer_context *ctx, const mer_scene_desc *scene, const float *eta, const float *wi, const float *u3, int64_t n,
                                 float *wo, float *weight, float *pdf);
/* PerspectiveCamera::sampleRay (src/sensors/perspective.cpp:247-269) */
int  mer_camera_rays(mer_context *ctx, const mer_scene_desc *scene, const float *pos2, int64_t n, float *o, float *d);
/* Sensor::sampleRay of the scene's sensor kind (perspective.cpp:247-269, orthographic.cpp:137-155, thinlens.cpp:293-322,
   telecentric.cpp:195-222): pos2[2*i..] = the film position in pixels, aperture2[2*i..] = the aperture sample in [0,1)^2 (read by the two
   lens kinds only; may be NULL for the other two); o, d [3*i..], mint, maxt [i].  The render kernels' own device function; for
   MER_SENSOR_PERSPECTIVE o and d are those of mer_camera_rays bit for bit. */
int  mer_sensor_rays(mer_context *ctx, const mer_scene_desc *scene, const float *pos2, const float *aperture2, int64_t n, float *o, float *d,
                     float *mint, float *maxt);
/* PerspectiveCamera::sampleDirect (src/sensors/perspective.cpp:387-424, importance :191-245) of the scene's pinhole at n reference points
   ref[3*i..]: out stride 8: value = importance x invDist^2, the film position in pixels [2], the unit direction from the point to the
   sensor [3], the distance, 0.  All zero for a point outside the clip range or the frustum.  cam_to_world must be rigid (its inverse is
   taken as the transpose).  The light tracer's own device function. */
int  mer_sensor_direct(mer_context *ctx, const mer_scene_desc *scene, const float *ref, int64_t n, float *out);
/* PerspectiveCamera::getSamplePosition (perspective.cpp:367-385) of n world directions dirs[3*i..] leaving the sensor (need not be unit):
   out_uv[2*i..] = the film position in pixels, out_ok[i] = 1, or 0 (and uv = 0) behind the sensor or outside the frame.  The light
   tracer's own device function: the pixel of a curved connection comes from its arrival direction through it. */
int  mer_sensor_position(mer_context *ctx, const mer_scene_desc *scene, const float *dirs, int64_t n, float *out_uv, int32_t *out_ok);
/* PathLengthSampler::correlationFunction for the scene's modulation (src/librender/pathlengthsampler.cpp:68-114) */
int  mer_correlation(mer_context *ctx, const mer_scene_desc *scene, const float *path_length, int64_t n, float *out);
/* per-path radiance Li of sample `sample_index` for every pixel: out[(y*w+x)*3] (no filter); integrator = volpath only */
int  mer_render_paths(mer_context *ctx, const mer_scene_desc *scene, int32_t sample_index, uint64_t seed, float *out_rgb);
/* sampler stream known answers */
int  mer_rng_floats(mer_context *ctx, uint64_t seed, uint32_t pixel, uint32_t sample, int32_t n, float *out);
/* synthetic fields of BASELINE.json's configs generated on the device:
   kind 0 = sigma_t density, 1 = linear RIF (y), 2 = radial RIF; returns a device pointer the caller frees
   with mer_device_free */
int  mer_synth_field_dev(mer_context *ctx, int32_t kind, int32_t N, float **data_dev);
int  mer_device_free(mer_context *ctx, void *ptr_dev);

/* ---- several GPUs in one process: replaces the reference's N local workers whose image blocks are merged by
        film->put under a mutex (src/librender/renderproc.cpp:142-149; worker count: src/mitsuba/mitsuba.cpp:281).
        A mer_multi owns one context per entry of device_ids and one host thread per context for the duration of a render.  Volumes are
        replicated (every device holds every grid); the sample space of a render is cut into one mer_shard per context
        (MER_SHARD_SAMPLES: sample s goes to context s mod n -- perfect balance, result independent of n up to summation order;
        MER_SHARD_TILES: the 32x32 image tiles, dealt on diagonals of the tile grid -- the reference's block partition); the films are then
        sum-reduced onto the first device: with RCCL (ncclReduce inside ncclGroupStart/End over a communicator made by ncclCommInitAll,
        librccl.so loaded at run time) when all devices are distinct, by peer copy + an add kernel otherwise (a device listed twice,
        e.g. {0, 0}, runs the whole code path on a one-GPU machine; RCCL refuses duplicate devices).  No other exchange: paths are
        independent. ---- */
typedef struct mer_multi mer_multi;
enum { MER_SHARD_SAMPLES = 0, MER_SHARD_TILES = 1 };
enum { MER_REDUCE_NONE = 0 /* one context */, MER_REDUCE_RCCL = 1, MER_REDUCE_PEER_COPY = 2 };
int  mer_multi_create(const int32_t *device_ids, int32_t n, mer_multi **out);
void mer_multi_destroy(mer_multi *m);
const char *mer_multi_last_error(mer_multi *m);          /* m may be NULL: error of a failed create */
int32_t mer_multi_size(mer_multi *m);
mer_context *mer_multi_context(mer_multi *m, int32_t i); /* context i (options, leaf calls); owned by m */
/* mer_context_set_option on every context */
int  mer_multi_set_option(mer_multi *m, const char *name, int64_t value);
/* mer_volume_upload / mer_volume_build_spline / mer_volume_destroy on every context; ONE handle, valid in all of them */
int  mer_multi_volume_upload(mer_multi *m, const mer_grid_desc *desc, const void *host_data, int32_t layout, mer_volume *out);
int  mer_multi_volume_build_spline(mer_multi *m, mer_volume v);
int  mer_multi_volume_destroy(mer_multi *m, mer_volume v);
/* mer_envmap_upload on every context; ONE handle, valid in all of them (mer_multi_volume_destroy frees it) */
int  mer_multi_envmap_upload(mer_multi *m, int32_t width, int32_t height, const float *rgb_host, mer_volume *out);
/* renders sample indices spp_begin .. spp_begin + spp_count - 1 of every pixel, sharded over the contexts, and returns the reduced film
   float[height][width][mer_film_channels] in film_host.  rccl: 1 = use RCCL when the devices allow it and the library initialises (default choice; peer copy + add otherwise --
   mer_multi_last_stats reports which), 0 = always peer copy + add, 2 = RCCL even for a single context (a one-rank communicator: exercises the library binding on one GPU). */
int  mer_multi_render(mer_multi *m, const mer_scene_desc *scene, int32_t shard_mode, int32_t spp_begin, int32_t spp_count, uint64_t seed,
                      int32_t rccl, float *film_host);
/* of the last mer_multi_render: how the films were reduced (MER_REDUCE_*), wall milliseconds of every context's render (n floats, may be
   NULL), of the reduction, and the counters summed over the contexts (may be NULL) */
int  mer_multi_last_stats(mer_multi *m, int32_t *reduce_path, float *render_ms, float *reduce_ms, uint64_t counters[MER_C_COUNT]);

#ifdef __cplusplus
}
#endif
#endif /* MER_H */
