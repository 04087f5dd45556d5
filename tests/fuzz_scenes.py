"""Seeded random scenes for the EXTRA kernels (the instances launch_render selects for an emitter list, an envmap, a modulation, a non-null
boundary BSDF, the signed-distance boundary or a sensor beside the pinhole): every switch that reaches them is drawn, and the refusals of
mer_scene.hip are respected BY CONSTRUCTION -- a switch is drawn from the values the switches before it leave open, never drawn freely and
then rejected.  The rules, in the order they are applied:
  - the analytic acoustic RIF has no signed-distance kernel: an acoustic scene draws its boundary among cube and sphere;
  - aggressive tracing is drawn only for a signed-distance boundary with curved rays; Simpson only for straight rays in a gridded sigma_t;
  - rectangles (add_rect) need straight rays, a cube or sphere and a null boundary BSDF; a list with a rectangle holds no point or spot
    outside the shape (emitter_list), so a scene first draws whether it has rectangles and then its other entries from what is left;
  - a rough boundary (refuse_inside_rough) takes no point or spot inside the shape;
  - an envmap entry comes with a zero env_radiance;
  - a modulation comes with the transient decomposition;
  - the RIF layout is never BRICK125 (not built with the signed-distance boundary).
A boundary with a BSDF under a black environment keeps max_depth away from 3: the light of an emitter then needs more vertices than that to
reach the sensor, and a black image checks nothing.
No GPU is needed to build a scene: tests/test_fuzz_scenes.py counts what 48 seeds cover."""
import numpy as np
from mitsubaer_amd import params as P, capi, synth

SIZES = [(17, 13), (24, 20), (33, 40), (48, 40)]
CAM = P.look_at([-3, 0, 0], [0, 0, 0], [0, 1, 0])
SDF_BOX = ([-1.2] * 3, [1.2] * 3)
# the RECT_ABOVE family: above the cube facing down; a smaller one below it that hides part of it; one under the cube facing up
RECT_ABOVE = np.array([[1.5, 0, 0, 0], [0, 0, -1, 2.5], [0, -1.5, 0, 0]], np.float64)
RECT_NEAR = np.array([[0.6, 0, 0, 0.8], [0, 0, -1, 1.6], [0, -0.6, 0, 0]], np.float64)
RECT_BELOW = np.array([[1.0, 0, 0, 0.3], [0, 0, 1, -2.0], [0, 1.0, 0, 0]], np.float64)
INSIDE = [[0.2, 0.3, -0.1], [-0.5, -0.4, 0.3], [0.1, -0.3, 0.4]]          # within 0.71 of the centre: inside every shape drawn here
OUTSIDE = [[0.3, 1.6, -0.4], [-1.6, 1.4, 0.4], [0.5, -1.8, 0.6]]
WEIGHTS = [0.5, 3.0, 1.0, 2.5, 1.5]                                       # no two entries of a list share a samplingWeight
MODULATIONS = [P.MODULATION_SINE, P.MODULATION_SQUARE, P.MODULATION_HAMILTONIAN, P.MODULATION_MSEQ, P.MODULATION_DEPTHSELECTIVE]
FILMS = ["steady", "transient", "bounce", "steady", "bounce", "modulated"]
SENSOR_TAGS = {P.SENSOR_PERSPECTIVE: "perspective", P.SENSOR_ORTHOGRAPHIC: "orthographic", P.SENSOR_THINLENS: "thinlens", P.SENSOR_TELECENTRIC: "telecentric"}
TAGS = sorted(SENSOR_TAGS.values()) + ["point_inside", "point_outside", "spot", "rectangle", "two_rectangles", "envmap", "hdielectric", "hroughdielectric",
                                       "sdf", "sphere", "curved_trilinear", "bspline", "acoustic", "transient", "bounce", "modulation", "grid_sigma"] \
    + ["%dx%d" % s for s in SIZES]


def _scaled(cam, s):
    m = np.asarray(cam, np.float64).copy()
    m[:3, :3] = m[:3, :3] * np.asarray(s, np.float64)[None, :]
    return m.astype(np.float32)


def envmap_image(bright=(2, 11)):
    """a 16 x 8 lat-long map: a dim gradient and one bright 2 x 2 texel group"""
    y, x = np.mgrid[0:8, 0:16].astype(np.float64)
    img = np.stack([0.05 + 0.1 * y / 8, 0.1 + 0.05 * x / 16, 0.15 - 0.1 * y / 8], axis=2)
    img[bright[0]:bright[0] + 2, bright[1]:bright[1] + 2] = [24.0, 20.0, 12.0]
    return img.astype(np.float32)


def random_extra_scene(seed):
    """-> (SceneParams, layout of the RIF grid, the set of feature tags drawn)"""
    r = np.random.RandomState(1000 + seed)
    pick = lambda *a: a[r.randint(len(a))]
    tags = set()
    # ---- image and sensor
    w, h = pick(*SIZES)
    tags.add("%dx%d" % (w, h))
    kw = dict(width=w, height=h, rfilter=pick(P.FILTER_BOX, P.FILTER_GAUSSIAN), rfilter_param=0.5, fov_x_deg=float(pick(50.0, 60.0, 95.84)))
    sensor = pick(P.SENSOR_PERSPECTIVE, P.SENSOR_ORTHOGRAPHIC, P.SENSOR_THINLENS, P.SENSOR_TELECENTRIC)
    tags.add(SENSOR_TAGS[sensor])
    extent = float(pick(1.3, 1.6))
    aperture = float(pick(0.1, 0.3))
    kw.update(sensor=sensor, cam_to_world=_scaled(CAM, (extent, extent, 1.0)) if sensor in (P.SENSOR_ORTHOGRAPHIC, P.SENSOR_TELECENTRIC) else CAM)
    if sensor in (P.SENSOR_THINLENS, P.SENSOR_TELECENTRIC):
        kw.update(aperture_radius=aperture, focus_distance=float(pick(3.0, 2.75)))      # the cube's centre is 3 from the sensor
    # ---- medium
    N = pick(12, 16)
    kw.update(phase=pick(P.PHASE_ISOTROPIC, P.PHASE_HG), g=float(pick(0.8, -0.4, 0.3)), max_depth=pick(-1, 3, 6), rr_depth=pick(2, 5, 50),
              hide_emitters=bool(pick(0, 0, 1)))
    rif = pick("const", "const", "const", "const", "trilinear", "trilinear", "bspline", "bspline", "acoustic", "acoustic")
    curved = rif != "const"
    stepper = pick(P.STEP_VERLET, P.STEP_RK4)
    grid_sigma = pick(0, 1)
    if grid_sigma:
        tags.add("grid_sigma")
        kw.update(sigma_mode=P.SIGMA_GRID, density=synth.density_field(N), density_scale=float(pick(2.0, 4.0)), tr_estimator=pick(P.TR_RATIO, P.TR_WOODCOCK2),
                  albedo=pick([0.9, 0.9, 0.9], [0.95, 0.8, 0.6]))
        if not curved and pick(0, 1, 1, 1):
            kw.update(method=P.METHOD_SIMPSON)
    else:
        kw.update(sigma_mode=P.SIGMA_HOMOGENEOUS, sigma_s=pick([0.5, 3.5, 7.5], [1.0, 1.0, 1.0]), sigma_a=pick([0.05] * 3, [0.0, 0.1, 0.3]))
    if rif == "trilinear":
        tags.add("curved_trilinear")
        kw.update(rif_mode=P.RIF_TRILINEAR, rif=pick(synth.linear_rif, synth.radial_rif)(N), stepper=stepper, stepsize=0.5 * 2.0 / (N - 1))
    elif rif == "bspline":
        tags.add("bspline")
        # the grid reaches 2.0: with 12 nodes a box of 1.3 or 1.5 leaves part of the shape outside the spline-safe region, where every trace fails
        # and the medium renders black (on the CPU oracle too)
        kw.update(rif_mode=P.RIF_BSPLINE3, rif=synth.radial_rif(N, (-2.0,) * 3, (2.0,) * 3), rif_aabb=([-2.0] * 3, [2.0] * 3), stepper=stepper, stepsize=0.5 * 2.0 / (N - 1))
    elif rif == "acoustic":
        tags.add("acoustic")
        kw.update(rif_mode=P.RIF_ACOUSTIC, ac_n_o=1.33, ac_n_max=0.08, ac_k_r=4.0, ac_mode=pick(0, 1, 2), stepper=stepper, stepsize=0.5 * 2.0 / 23)
    # ---- boundary
    boundary = pick("cube", "sphere") if rif == "acoustic" else pick("cube", "cube", "sphere", "sdf")
    if boundary == "sphere":
        tags.add("sphere")
        kw.update(boundary=P.BOUNDARY_SPHERE, sph_radius=float(pick(0.8, 0.9)))
    elif boundary == "sdf":
        tags.add("sdf")
        kw.update(boundary=P.BOUNDARY_SDF, sdf=-synth.sphere_sdf(32, radius=0.9, aabb_min=SDF_BOX[0], aabb_max=SDF_BOX[1]), sdf_aabb=SDF_BOX)
        if curved and pick(0, 1, 1, 1):
            kw.update(aggressive_tracing=True)
    bsdf = pick(P.BSDF_NULL, P.BSDF_NULL, P.BSDF_NULL, P.BSDF_HDIELECTRIC, P.BSDF_HROUGHDIELECTRIC)
    if bsdf != P.BSDF_NULL:
        tags.add("hdielectric" if bsdf == P.BSDF_HDIELECTRIC else "hroughdielectric")
        kw.update(boundary_bsdf=bsdf)
        if not curved:
            kw.update(rif_const=1.33)
    if bsdf == P.BSDF_HROUGHDIELECTRIC:
        kw.update(rough_alpha=float(pick(0.05, 0.2)), rough_sample_visible=bool(pick(0, 1)),
                  rough_distribution=pick(P.MICROFACET_BECKMANN, P.MICROFACET_GGX, P.MICROFACET_PHONG))
    # ---- emitters: what the switches above leave open
    rects_possible = not curved and boundary != "sdf" and bsdf == P.BSDF_NULL
    n_rects = pick(0, 1, 2, 2) if rects_possible else 0
    menu = []
    if bsdf != P.BSDF_HROUGHDIELECTRIC:
        menu += ["point_inside", "spot_inside"]
    if n_rects == 0:
        menu += ["point_outside", "spot_outside"]
    envmap = pick(0, 0, 1)
    n_other = pick(1, 2, 3) if n_rects + envmap else pick(1, 2, 3, 4)
    n_other = min(n_other, 5 - n_rects - envmap)
    first = r.randint(len(WEIGHTS))
    weight = lambda: WEIGHTS[(first + len(ems)) % len(WEIGHTS)]
    ems = []
    if n_rects:
        tags.add("rectangle")
        rects = [pick(RECT_ABOVE, RECT_BELOW, RECT_NEAR)] if n_rects == 1 else [RECT_ABOVE, pick(RECT_NEAR, RECT_BELOW)]
        if n_rects == 2:
            tags.add("two_rectangles")
        for m in rects:
            ems.append(P.area_emitter(m, pick([3.0, 2.0, 1.0], [1.0, 2.0, 4.0]), weight()))
    for _ in range(n_other):
        kind = pick(*menu)
        k = r.randint(3)
        inten = pick([1.0, 0.8, 0.5], [1.0, 0.5, 2.0])
        cutoff = float(pick(20.0, 60.0, 180.0))
        beam = pick(None, 0.5 * cutoff)
        if kind.startswith("point"):
            tags.add(kind)
            ems.append(P.point_emitter((INSIDE if kind == "point_inside" else OUTSIDE)[k], inten, weight()))
        else:
            tags.add("spot")
            pos = (INSIDE if kind == "spot_inside" else OUTSIDE)[k]
            target = INSIDE[(k + 1) % 3]                                     # aimed across the shape, never along a coordinate axis
            ems.append(P.spot_emitter(P.look_at(pos, target, [0.2, 1.0, 0.1]), inten, cutoff, beam, weight()))
    if envmap:
        tags.add("envmap")
        ems.insert(r.randint(len(ems) + 1), P.envmap_emitter(envmap_image(pick((2, 11), (5, 3))), P.rotation(pick([0.3, 1.0, -0.4], [1.0, 0.2, 0.1]), float(pick(57.0, 140.0))),
                                                            float(pick(1.0, 0.5)), weight()))
        kw.update(env_radiance=[0.0, 0.0, 0.0])
    else:
        kw.update(env_radiance=pick([0.0, 0.0, 0.0], [0.5, 0.7, 0.9], [1.0, 1.0, 1.0]))
    kw.update(emitters=ems)
    if bsdf != P.BSDF_NULL and not envmap and kw["env_radiance"] == [0.0, 0.0, 0.0] and kw["max_depth"] == 3:
        kw.update(max_depth=6)
    # ---- film
    film = pick(*FILMS)
    frames = pick(16, 32, 64)
    if film == "transient":
        tags.add("transient")
        kw.update(decomposition=P.DECOMPOSITION_TRANSIENT, min_bound=0.0, max_bound=16.0, bin_width=16.0 / frames, calibrated_transient=bool(pick(0, 1)))
    elif film == "bounce":
        tags.add("bounce")
        kw.update(decomposition=P.DECOMPOSITION_BOUNCE, min_bound=0.0, max_bound=16.0, bin_width=1.0)
    elif film == "modulated":
        tags.add("modulation")
        kw.update(decomposition=P.DECOMPOSITION_TRANSIENT, min_bound=0.0, max_bound=16.0, bin_width=16.0 / frames, modulation=pick(*MODULATIONS),
                  mod_lambda=2.3, mod_phase_deg=25.0, mod_P=8)
    layout = pick(capi.LAYOUT_DENSE, capi.LAYOUT_CELL8, capi.LAYOUT_BRICK27, capi.LAYOUT_AUTO)
    return P.SceneParams(**kw), layout, tags


def connect_stage(p):
    """launch_render's rule: a curved-ray connection stage runs for a point or a spot unless the boundary is rough"""
    return p.rif_mode != P.RIF_CONST and p.boundary_bsdf != P.BSDF_HROUGHDIELECTRIC and any(e["type"] in (P.EMITTER_POINT, P.EMITTER_SPOT) for e in p.emitters)


def one_frame_box_seeds(seeds):
    """the seeds whose scene has the box filter and a film of one frame (steady state or modulated): a splat stays in its pixel"""
    out = []
    for s in seeds:
        p, _, _ = random_extra_scene(s)
        if p.rfilter == P.FILTER_BOX and (p.decomposition == P.DECOMPOSITION_NONE or p.modulation != P.MODULATION_NONE):
            out.append(s)
    return out


BOUNDS_SEEDS = [1, 2, 3, 6, 9, 15, 16, 21, 24, 25, 37, 44]          # between them every tag (tests/test_fuzz_scenes.py)
LEAK_SEEDS = [7, 16, 10, 33, 13, 9]                                   # consecutive scenes share no filter, sensor, film depth or envmap


def film_frames(p):
    """the frames of the scene's film (film_frames of mer_scene.hip): its channels are 3 x this + 2"""
    if p.decomposition == P.DECOMPOSITION_NONE or p.modulation != P.MODULATION_NONE:
        return 1
    return int(np.ceil((p.max_bound - p.min_bound) / p.bin_width))
