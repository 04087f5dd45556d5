"""Light tracing on the GPU (mer_scene_desc.integrator = MER_INTEGRATOR_PTRACER, mer_ptracer.hpp): the two leaf entry points of the sensor
connection against float64 restatements; the once-scattered light of a collimated beam against the float64 quadrature of
tests/ptracer64.py, per pixel and per transient frame; light tracing against path tracing (volpath on the GPU) and against the float64
light tracer; the curved geometry -- a vertex lands on the pixel its connection ARRIVES at -- against a float64 shooting through a
linear index field; the film contract, the shards, and the refusals.

Statistics: films of 24 x 20 pixels, variances from K = 16 independent renders with different seeds (64 where volpath is the other side), the project's bar -- at most 1 + 1 %
of the pixels (frames) beyond 4 sigma, and the film total within 4 sigma."""
import os
import numpy as np
import pytest
from mitsubaer_amd import params as P, capi, host, synth
from tests import scenes
from tests import ptracer64 as pt
from tests import test_ptracer64 as T64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, FOV, CAM = T64.W, T64.H, T64.FOV, T64.CAM
K = 16


def _beam_frame(origin, direction):
    return P.look_at(origin, np.asarray(origin, np.float64) + np.asarray(direction, np.float64), [0, 1, 0] if abs(direction[1]) < 0.9 else [1, 0, 0])


def _base(**kw):
    """the scene of tests/test_ptracer64.py: grey homogeneous medium, HG, box filter, the beam of power 5"""
    base = dict(w=W, h=H, fov_x_deg=FOV, cam_to_world=CAM, phase=P.PHASE_HG, g=T64.G, sigma_s=[T64.SIGMA_S] * 3, sigma_a=[T64.SIGMA_A] * 3,
                env_radiance=[0, 0, 0], rfilter=P.FILTER_BOX, rfilter_param=0.5, integrator=P.INTEGRATOR_PTRACER,
                emitters=[P.collimated_emitter(_beam_frame(T64.BEAM_O, T64.BEAM_D), [T64.POWER] * 3)])
    base.update(kw)
    return scenes.homogeneous_scene(**base)


def _renders(ctx, p, spp, seed0, k=K, layout=capi.LAYOUT_DENSE):
    """k independent renders: (k, H, W, frames, 3) RGB / weight, and the last raw film"""
    sc, vols = ctx.upload_scene(p, layout=layout)
    out = []
    for j in range(k):
        f = ctx.render_to_host(sc, 0, spp, seed=seed0 + j)
        assert np.isfinite(f).all()
        rgb = f[..., :-2].reshape(f.shape[0], f.shape[1], -1, 3)
        out.append(rgb / f[..., -1][..., None, None])
    for v in vols:
        v.destroy()
    return np.array(out), f


def _bar(mean, sd, ref, ref_var=0.0, what=""):
    """the project's bar for `mean` (standard deviation of the mean `sd`) against `ref` (variance ref_var): (pixels beyond 4 sigma, max z)"""
    s = np.sqrt(sd * sd + ref_var)
    floor = 1e-7 * max(float(np.abs(ref).max()), 1e-30)
    z = np.abs(mean - ref) / np.maximum(s, floor)
    print("%s: %d of %d beyond 4 sigma, max z %.2f" % (what, (z > 4).sum(), z.size, z.max()))
    assert (z > 4).sum() <= 1 + 0.01 * z.size, (what, np.sort(z.ravel())[-5:])
    return z


def _total_bar(totals, ref, ref_var=0.0, what=""):
    zt = abs(totals.mean() - ref) / np.sqrt(totals.var(ddof=1) / len(totals) + ref_var)
    print("%s: total z %.2f" % (what, zt))
    assert zt <= 4, (what, zt)


# ---- 1. the leaves ---------------------------------------------------------------------------------------------------------------------

LEAF_CAM = P.look_at([-3.0, 0.5, 0.4], [0.1, -0.1, 0.0], [0, 1, 0])
NEAR, FAR = 0.5, 4.5


def _direct(cam, w, h, fov, near, far, ref, dt):
    """PerspectiveCamera::sampleDirect restated in the precision dt: (n, 7) value, u, v, d, dist; and the margin by which the point is
    inside (> 0) or outside (< 0) the clip range and the frame"""
    f = dt
    m = np.asarray(cam, f); R, o = m[:3, :3], m[:3, 3]
    v = np.asarray(ref, f) - o
    loc = (v @ R).astype(f)
    z = loc[:, 2]
    tan = f(np.tan(np.radians(f(fov)) / f(2))); aspect = f(w) / f(h)
    zs = np.where(np.abs(z) > 0, z, f(1))
    u = f(0.5) - f(0.5) * (loc[:, 0] / zs) / tan; t = f(0.5) - f(0.5) * (loc[:, 1] / zs) * aspect / tan
    margin = np.minimum.reduce([z - f(near), f(far) - z, u, f(1) - u, t, f(1) - t])
    ok = margin >= 0
    r = np.sqrt((loc * loc).sum(1)).astype(f)
    cos = np.where(ok, z / r, f(1))
    area = (f(2) * tan) ** 2 / aspect
    val = np.where(ok, f(1) / (area * cos * cos * cos) / (r * r), f(0))
    d = -v / r[:, None]
    out = np.column_stack([val, u * f(w), t * f(h), d, r]).astype(f)
    out[~ok] = 0
    return out, margin


def test_sensor_direct_matches_float64(ctx):
    """mer_sensor_direct against the float64 restatement at 20 000 points around the frustum (a third of them inside); the rule of
    test_area_direct_matches_float64: per column, the GPU's largest deviation from float64 is at most 4 x that of the same formulas in
    numpy float32.  Points behind the camera, outside the clip range or outside the frame give exactly 0 in every column.
    Measured maxima |deviation from float64|, numpy float32 | GPU: see the table this test prints (recorded in DESIGN.md)."""
    p = _base(w=W, h=H, cam_to_world=LEAF_CAM, near_clip=NEAR, far_clip=FAR, fov_x_deg=50.0)
    sc, _ = ctx.upload_scene(p)
    rng = np.random.default_rng(11)
    n = 20000
    # camera-space depths from behind the sensor to beyond the far plane, lateral positions up to 1.6 x the frame's half extent
    zc = rng.uniform(-1.5, 6.0, n); tx = np.tan(np.radians(25.0)); ty = tx * H / W
    local = np.stack([rng.uniform(-1.6, 1.6, n) * tx * np.abs(zc), rng.uniform(-1.6, 1.6, n) * ty * np.abs(zc), zc], 1)
    ref = (np.asarray(LEAF_CAM, np.float64)[:, 3] + local @ np.asarray(LEAF_CAM, np.float64)[:, :3].T).astype(np.float32)
    got = ctx.sensor_direct(sc, ref).astype(np.float64)
    r64, margin = _direct(LEAF_CAM, W, H, 50.0, NEAR, FAR, ref, np.float64)
    r32, _ = _direct(LEAF_CAM, W, H, 50.0, NEAR, FAR, ref, np.float32)
    clear = np.abs(margin) > 1e-4
    inside = clear & (margin > 0)
    loc = (ref.astype(np.float64) - np.asarray(LEAF_CAM, np.float64)[:, 3]) @ np.asarray(LEAF_CAM, np.float64)[:, :3]
    assert inside.sum() > n // 10 and (clear & (loc[:, 2] < 0)).sum() > 1000 and (clear & (loc[:, 2] > FAR)).sum() > 100
    assert (clear & (loc[:, 2] > NEAR) & (loc[:, 2] < FAR) & ~inside).sum() > 1000           # inside the clip range, outside the frame
    assert np.all(got[clear & ~inside] == 0)
    assert np.all(got[inside, 0] > 0) and np.all(got[:, 7] == 0)
    bad = []
    for name, cols in (("value", [0]), ("uv", [1, 2]), ("d", [3, 4, 5]), ("dist", [6])):
        e32 = np.abs(r32[inside][:, cols].astype(np.float64) - r64[inside][:, cols]).max()
        eg = np.abs(got[inside][:, cols] - r64[inside][:, cols]).max()
        print("%-6s numpy float32 %.3e | GPU %.3e" % (name, e32, eg))
        if eg > 4 * e32:
            bad.append((name, e32, eg))
    assert not bad, bad


def test_sensor_position_inverts_camera_rays(ctx):
    """getSamplePosition(sampleRay(pos).d) = pos to within 1e-3 pixel over the whole film; a direction behind the sensor or outside the
    frame is refused.  Measured (MI355X): largest deviation 7.6e-06 px."""
    p = _base(cam_to_world=LEAF_CAM, fov_x_deg=50.0)
    sc, _ = ctx.upload_scene(p)
    rng = np.random.default_rng(12)
    pos = (rng.random((20000, 2)) * [W, H]).astype(np.float32)
    o, d = ctx.camera_rays(sc, pos)
    uv, ok = ctx.sensor_position(sc, d * rng.uniform(0.5, 3.0, (len(d), 1)).astype(np.float32))       # any length
    assert ok.all()
    print("largest |uv - pos| %.3e px" % np.abs(uv - pos).max())
    assert np.abs(uv - pos).max() < 1e-3
    uv, ok = ctx.sensor_position(sc, -d)
    assert not ok.any() and np.all(uv == 0)
    outside = (np.array([[-0.2 * W, 0.5 * H], [1.2 * W, 0.5 * H], [0.5 * W, -0.2 * H], [0.5 * W, 1.2 * H]])).astype(np.float32)
    _, d2 = ctx.camera_rays(sc, outside)
    uv, ok = ctx.sensor_position(sc, d2)
    assert not ok.any()


# ---- 2. a collimated beam, once scattered, against the quadrature ----------------------------------------------------------------------

def test_collimated_single_scattering_matches_the_quadrature(ctx):
    """max_depth 3 is black, 4 is the once-scattered light: per pixel against tests/ptracer64.single_scatter_quadrature.
    Measured (MI355X): printed below."""
    r, film = _renders(ctx, _base(max_depth=3), 4, 100, k=2)
    assert not r.any() and np.all(film[..., -1] == 4) and np.all(film[..., -2] == 4)
    q = T64.quadrature()[..., 0]
    r, _ = _renders(ctx, _base(max_depth=4), 32, 200)
    np.testing.assert_allclose(r[..., 1], r[..., 0], rtol=1e-5, atol=1e-9)                         # a grey scene (the three channels' atomics add in their own order)
    g = r[:, :, :, 0, 0]
    _bar(g.mean(0), g.std(0, ddof=1) / np.sqrt(K), q, what="pixels")
    assert ((g.mean(0) > 0) == (q > 0)).mean() > 0.99
    _total_bar(g.sum((1, 2)), q.sum(), what="film")


def test_collimated_transient_frames_match_the_quadrature(ctx):
    """the same on a transient film: per-frame totals against the quadrature restricted by s + r (emitter edge + in-medium edge + connection
    edge + camera edge).  Measured (MI355X): 0 of 10 frames beyond 4 sigma, largest z 1.31."""
    lo, hi, bw = T64.TRANSIENT
    q = T64.quadrature(T64.TRANSIENT).sum((0, 1))
    r, film = _renders(ctx, _base(max_depth=4, decomposition=P.DECOMPOSITION_TRANSIENT, min_bound=lo, max_bound=hi, bin_width=bw), 32, 300)
    assert film.shape[-1] == len(q) * 3 + 2
    g = r[..., 0].sum((1, 2))                                       # (K, frames)
    _bar(g.mean(0), g.std(0, ddof=1) / np.sqrt(K), q, what="frames")
    assert np.array_equal(g.mean(0) > 0, q > 0)
    # calibrated: the camera edge (cube face -> pinhole: 2 / cos) leaves the path length, the light arrives ~2.0 - 2.1 earlier
    rc, _ = _renders(ctx, _base(max_depth=4, decomposition=P.DECOMPOSITION_TRANSIENT, min_bound=lo - 2.0, max_bound=hi - 2.0, bin_width=bw, calibrated_transient=True), 32, 300, k=2)
    gc = rc[..., 0].sum((0, 1, 2))
    assert abs(np.average(np.arange(len(q)), weights=gc) - np.average(np.arange(len(q)), weights=q)) < 0.5


# ---- 3. light tracing = path tracing ---------------------------------------------------------------------------------------------------

PIN, I_PIN = [0.05, -0.04, 0.02], 2.0      # near the centre: volpath's curved connections to it rarely leave the cube (see the test's docstring)
SPOT_POS = np.array([0.3, 2.5, -0.4])


def _spot():
    z = np.array([0.1, 0.0, 0.0]) - SPOT_POS; z /= np.linalg.norm(z)
    x = np.cross([0.0, 0.0, 1.0], z); x /= np.linalg.norm(x)
    M = np.zeros((3, 4)); M[:, 0] = x; M[:, 1] = np.cross(z, x); M[:, 2] = z; M[:, 3] = SPOT_POS
    return P.spot_emitter(M, [6.0] * 3, 25.0, 15.0)


EMITTERS = {"point_inside": lambda: P.point_emitter(PIN, [I_PIN] * 3), "spot_outside": _spot}


def _medium(name):
    if name == "homogeneous":
        return dict()
    if name == "grid16":
        return dict(sigma_mode=P.SIGMA_GRID, density=synth.density_field(16), density_scale=3.0, albedo=[0.8] * 3, tr_estimator=P.TR_RATIO)
    return dict(rif_mode=P.RIF_TRILINEAR, rif=np.ones((6, 6, 6), np.float32), stepsize=0.05, stepper=P.STEP_VERLET if name == "curved_verlet" else P.STEP_RK4)


@pytest.mark.parametrize("max_depth", [2, 3, -1])
@pytest.mark.parametrize("medium", ["homogeneous", "grid16", "curved_verlet", "curved_rk4"])
@pytest.mark.parametrize("emitter", sorted(EMITTERS))
def test_light_tracing_equals_path_tracing(ctx, emitter, medium, max_depth):
    """ptracer against volpath on the GPU, the same scene and depth limit: two estimators of one image.  max_depth 2 is black for both (a
    vertex needs depth 2 and its connection one more).  With straight rays 3 is the once-scattered light of the emitter inside the cube and
    still black for the spot outside it (both integrators count the null crossing of the connection); through the curved kernels both charge
    a path one crossing at most, so the spot's once-scattered light is there at 3 in both.  -1 is everything.  Homogeneous sigma, a 16^3
    sigma_t grid, and the curved kernels (Walk and the connection solver) on an index field that is 1 everywhere, with both steppers.  The
    homogeneous point-emitter case is also held against the float64 light tracer.
    Measured (MI355X), pixels beyond 4 sigma of 480 | largest z | z of the film total:
        point inside   homogeneous  depth 3: 1 | 4.10 | 0.86      depth -1: 0 | 3.32 | 0.79     (against ptracer64: 0 | 3.23 and 0 | 3.12)
                       16^3 grid    depth 3: 0 | 3.26 | 0.06      depth -1: 1 | 4.59 | 0.93
                       curved       depth 3: 0 | 3.24 - 3.46 | 2.09 - 2.34      depth -1: 0 - 1 | 3.84 - 4.60 | 1.43 - 1.44
        spot outside   homogeneous  depth -1: 0 | 3.40 | 0.72     16^3 grid depth -1: 0 | 3.94 | 0.36     curved depth -1: 0 | 2.90 - 2.95 | 0.13 - 0.17
    With 16 renders of 32 samples on either side the same comparison showed up to 14 pixels beyond 4 sigma for the emitter inside the cube:
    volpath's variance estimate, not the light tracer (see the comment below)."""
    # 64 renders per estimator.  Volpath's own estimate of an emitter INSIDE the medium has no finite variance (its 1 / r^2 emitter samples at
    # vertices that fall near the emitter), so a variance taken from its renders is too small wherever no such vertex fell; with straight
    # rays it gets 32 x the light tracer's samples, so that the light tracer's (bounded, well-behaved) spread is the one that sets sigma
    spp = 64
    spp_volpath = 64 if medium.startswith("curved") else 2048
    KE = 64
    kw = dict(emitters=[EMITTERS[emitter]()], max_depth=max_depth, **_medium(medium))
    lt, film = _renders(ctx, _base(**kw), spp, 1000, k=KE)
    assert np.all(film[..., -1] == spp)
    ptr, _ = _renders(ctx, _base(integrator=P.INTEGRATOR_VOLPATH, **kw), spp_volpath, 2000, k=KE)
    a, b = lt[:, :, :, 0, 0], ptr[:, :, :, 0, 0]
    black = max_depth == 2 or (max_depth == 3 and emitter == "spot_outside" and not medium.startswith("curved"))
    if black:
        print("%s %s depth %d: film totals ptracer %.5g, volpath %.5g" % (emitter, medium, max_depth, a.sum((1, 2)).mean(), b.sum((1, 2)).mean()))
        assert not a.any() and not b.any()
        return
    assert a.mean(0).sum() > 0 and b.mean(0).sum() > 0
    what = "%s %s depth %d" % (emitter, medium, max_depth)
    print("%s: film totals ptracer %.5g +- %.2g, volpath %.5g +- %.2g" % (what, a.sum((1, 2)).mean(), a.sum((1, 2)).std(ddof=1) / np.sqrt(KE),
                                                                      b.sum((1, 2)).mean(), b.sum((1, 2)).std(ddof=1) / np.sqrt(KE)))
    _total_bar(a.sum((1, 2)), b.sum((1, 2)).mean(), b.sum((1, 2)).var(ddof=1) / KE, what=what)
    _bar(a.mean(0), a.std(0, ddof=1) / np.sqrt(KE), b.mean(0), b.var(0, ddof=1) / KE, what=what)
    if emitter == "point_inside" and medium == "homogeneous":
        # 64 samples per batch: with fewer, the dim pixels at the film's edge hold a handful of contributions per batch and their spread is not Gaussian
        m64, v64 = pt.render(pt.point(PIN, I_PIN), T64.SIGMA_S, T64.SIGMA_A, T64.G, W, H, FOV, CAM, spp=2048, batches=32, seed=7, max_depth=max_depth)
        _bar(a.mean(0), a.std(0, ddof=1) / np.sqrt(KE), m64[..., 0], v64[..., 0], what=what + " vs ptracer64")


# ---- 4. curved geometry: the pixel of the arrival direction ----------------------------------------------------------------------------

RIF_A, RIF_B = 1.3, 0.15                      # n = 1.3 + 0.15 y, exact under trilinear interpolation on any grid
CW, CH, CFOV = 48, 40, 60.0
CCAM = P.look_at([-2.0, 0.2, 0.0], [0.0, 0.2, 0.0], [0, 1, 0])
CBEAM_O, CBEAM_D = np.array([0.2, -0.3, -3.0]), np.array([0.0, 0.0, 1.0])


def _rk4(p, v, h):
    """one RK4 step of dp/ds = v / n, dv/ds = grad n for n = RIF_A + RIF_B y (float64)"""
    def f(p, v):
        return v / (RIF_A + RIF_B * p[1]), np.array([0.0, RIF_B, 0.0])
    k1p, k1v = f(p, v); k2p, k2v = f(p + 0.5 * h * k1p, v + 0.5 * h * k1v); k3p, k3v = f(p + 0.5 * h * k2p, v + 0.5 * h * k2v); k4p, k4v = f(p + h * k3p, v + h * k3v)
    return p + h / 6 * (k1p + 2 * k2p + 2 * k3p + k4p), v + h / 6 * (k1v + 2 * k2v + 2 * k3v + k4v)


def _march_to(p, v, axis, target, h=0.01):
    """follow the ray until coordinate `axis` reaches `target` (it moves monotonically toward it); the last step is shortened by bisection"""
    sgn = np.sign(target - p[axis])
    for _ in range(100000):
        q, w = _rk4(p, v, h)
        if sgn * (q[axis] - target) >= 0:
            lo, hi = 0.0, h
            for _ in range(60):
                mid = 0.5 * (lo + hi)
                q, w = _rk4(p, v, mid)
                if sgn * (q[axis] - target) >= 0:
                    hi = mid
                else:
                    lo = mid
            return q, w
        p, v = q, w
    raise AssertionError("ray never reached the plane")


def _camera_ray_hits(ab, cam):
    """the ray that leaves the pinhole along the camera-space direction (a, b, 1): refracted into the cube at the face x = -1 (Snell, index 1
    outside), followed through the index field: returns a function plane x -> point"""
    R, o = np.asarray(cam, np.float64)[:, :3], np.asarray(cam, np.float64)[:, 3]
    d = R @ np.array([ab[0], ab[1], 1.0]); d /= np.linalg.norm(d)
    pb = o + d * ((-1.0 - o[0]) / d[0])
    n2 = RIF_A + RIF_B * pb[1]
    vt = d - d[0] * np.array([1.0, 0, 0])
    v = vt + np.sqrt(n2 * n2 - vt @ vt) * np.array([1.0, 0, 0])
    return pb, v


def _curved_prediction(npts=64):
    """the beam by RK4; for npts beam points the pinhole direction whose refracted, curved ray passes through the point (Newton on the two
    direction parameters, finite-difference Jacobian); the film positions of those ARRIVAL directions (`curve`), and the straight-line
    projections of the same points (`straight`)"""
    cam = pt.Pinhole(CCAM, CW, CH, CFOV)
    # the beam: straight to the face z = -1 (the null boundary does not refract it), then through the field
    p = CBEAM_O + CBEAM_D * ((-1.0 - CBEAM_O[2]) / CBEAM_D[2])
    v = CBEAM_D * (RIF_A + RIF_B * p[1])
    zs = np.linspace(-0.97, 0.97, npts)
    pts = []
    for z in zs:
        p, v = _march_to(p, v, 2, z)
        pts.append(p.copy())
    pts = np.array(pts)
    assert np.all(np.abs(pts) < 1)
    curve = []
    for q in pts:
        loc = (q - cam.o) @ cam.R
        ab = np.array([loc[0] / loc[2], loc[1] / loc[2]])                 # start: the straight line
        for _ in range(30):
            def res(ab):
                pb, vv = _camera_ray_hits(ab, CCAM)
                e, _ = _march_to(pb, vv, 0, q[0])
                return e[1:] - q[1:]
            r0 = res(ab)
            if np.abs(r0).max() < 1e-10:
                break
            J = np.column_stack([(res(ab + [1e-6, 0]) - r0) / 1e-6, (res(ab + [0, 1e-6]) - r0) / 1e-6])
            ab = ab - np.linalg.solve(J, r0)
        else:
            raise AssertionError("shooting did not converge")
        curve.append([0.5 * (1 - ab[0] / cam.tan) * CW, 0.5 * (1 - ab[1] * cam.aspect / cam.tan) * CH])
    _, uv, _, _ = cam.connect(pts)
    return {"points": pts, "curve": np.array(curve), "straight": uv}


def _dist_to_polyline(q, poly):
    a, b = poly[:-1], poly[1:]
    t = np.clip(((q - a) * (b - a)).sum(1) / ((b - a) ** 2).sum(1), 0, 1)
    return np.linalg.norm(a + t[:, None] * (b - a) - q, axis=1).min()


def test_curved_connections_land_on_the_arrival_pixel(ctx):
    """n = 1.3 + 0.15 y on a 5^3 dense grid, a collimated beam, single scattering (max_depth 3: through the curved kernels a path is charged
    one null crossing at most, so 3 is the once-scattered light and 4 would add the twice-scattered), 48 x 40 box film.  Every pixel that holds more than 1 % of
    the film lies within 1.5 px of the curve the float64 shooting predicts; the straight-line projection of the same beam points runs more
    than 3 px beside that curve (checked here, so that a tracer that took the pixel from sampleDirect's uv would fail).
    Measured (MI355X): the straight-line projection runs up to 5.00 px beside the curve; 31 bright pixels, the farthest 1.01 px from the
    predicted curve and 5.82 px from the straight-line projection."""
    c = _curved_prediction()
    off = np.linalg.norm(c["curve"] - c["straight"], axis=1)
    print("straight-line projection off the curve by up to %.2f px" % off.max())
    assert off.max() > 3.0
    assert c["curve"][:, 0].min() > 1 and c["curve"][:, 0].max() < CW - 1 and c["curve"][:, 1].min() > 1 and c["curve"][:, 1].max() < CH - 1
    yy = np.linspace(-1, 1, 5)
    rif = np.broadcast_to((RIF_A + RIF_B * yy)[None, :, None], (5, 5, 5)).astype(np.float32).copy()
    p = _base(w=CW, h=CH, fov_x_deg=CFOV, cam_to_world=CCAM, max_depth=3, rif_mode=P.RIF_TRILINEAR, rif=rif, stepsize=0.02, stepper=P.STEP_RK4,
              emitters=[P.collimated_emitter(_beam_frame(CBEAM_O, CBEAM_D), [5.0] * 3)])
    sc, vols = ctx.upload_scene(p, layout=capi.LAYOUT_DENSE)
    f = ctx.render_to_host(sc, 0, 16, seed=5)
    assert np.isfinite(f).all() and np.all(f[..., 4] == 16)
    img = f[..., 0]
    assert img.sum() > 0
    ys, xs = np.nonzero(img > 0.01 * img.sum())
    assert len(ys) >= 10
    d = np.array([_dist_to_polyline(np.array([x + 0.5, y + 0.5]), c["curve"]) for x, y in zip(xs, ys)])
    ds = np.array([_dist_to_polyline(np.array([x + 0.5, y + 0.5]), c["straight"]) for x, y in zip(xs, ys)])
    print("bright pixels: %d, farthest from the predicted curve %.2f px (from the straight-line projection: %.2f px)" % (len(d), d.max(), ds.max()))
    assert d.max() <= 1.5
    for v in vols:
        v.destroy()


# ---- 5. film and sharding --------------------------------------------------------------------------------------------------------------

def _point_scene(**kw):
    return _base(emitters=[P.point_emitter(PIN, [I_PIN] * 3), EMITTERS["spot_outside"]()], max_depth=8, **kw)


def test_decomposed_frames_sum_to_the_steady_film(ctx):
    """same seed, same paths: the transient and the bounce frames add up to the steady film; alpha and weight are S everywhere"""
    S = 8
    sc, _ = ctx.upload_scene(_point_scene())
    steady = ctx.render_to_host(sc, 0, S, seed=9)
    assert steady[..., :3].sum() > 0 and np.all(steady[..., 3] == S) and np.all(steady[..., 4] == S)
    for kw in (dict(decomposition=P.DECOMPOSITION_TRANSIENT, min_bound=0.0, max_bound=64.0, bin_width=1.0),
               dict(decomposition=P.DECOMPOSITION_BOUNCE, min_bound=0.0, max_bound=16.0, bin_width=1.0)):
        sc, _ = ctx.upload_scene(_point_scene(**kw))
        f = ctx.render_to_host(sc, 0, S, seed=9)
        frames = f[..., :-2].reshape(H, W, -1, 3)
        assert (frames.sum((0, 1, 3)) > 0).sum() >= 3
        np.testing.assert_allclose(frames.sum(2), steady[..., :3], rtol=1e-4, atol=1e-5)
        assert np.all(f[..., -1] == S) and np.all(f[..., -2] == S)
    # a modulated film is one frame: the steady film weighted by the correlation function, here a constant 1 (lambda far above any path)
    sc, _ = ctx.upload_scene(_point_scene(decomposition=P.DECOMPOSITION_TRANSIENT, min_bound=0.0, max_bound=64.0, bin_width=1.0,
                                          modulation=P.MODULATION_SINE, mod_lambda=1e9, mod_phase_deg=0.0))
    f = ctx.render_to_host(sc, 0, S, seed=9)
    assert f.shape[-1] == 5
    np.testing.assert_allclose(f[..., :3], steady[..., :3], rtol=1e-4, atol=1e-5)


def test_shards_add_up_to_the_whole(ctx):
    """two sample shards, and four tile shards (a 40 x 36 film: 2 x 2 tiles, three of them partial), add up to the unsharded film; splats
    land on any pixel, the weights on the shard's own"""
    p = _point_scene(w=40, h=36)
    sc, _ = ctx.upload_scene(p)
    whole = ctx.render_to_host(sc, 0, 8, seed=4)
    assert np.all(whole[..., 4] == 8)
    parts = [ctx.render_to_host(sc, b, 4, seed=4, spp_stride=2) for b in (0, 1)]
    assert np.all(parts[0][..., 4] == 4)
    np.testing.assert_allclose(parts[0] + parts[1], whole, rtol=1e-4, atol=1e-5)
    tiles = [ctx.render_to_host(sc, 0, 8, seed=4, tile_rank=r, tile_count=4) for r in range(4)]
    for t in tiles:
        assert set(np.unique(t[..., 4])) == {0.0, 8.0}                 # a shard's weights lie on its own tiles ...
        assert (t[..., :3].sum(2) > 0).sum() > (t[..., 4] > 0).sum()      # ... its splats anywhere
    np.testing.assert_allclose(sum(tiles), whole, rtol=1e-4, atol=1e-5)


def test_two_contexts_match_one(ctx):
    p = _point_scene(w=40, h=36)
    sc, _ = ctx.upload_scene(p)
    one = ctx.render_to_host(sc, 0, 8, seed=6)
    m = capi.MultiContext([0, 0])
    try:
        for mode in (capi.SHARD_SAMPLES, capi.SHARD_TILES):
            s2, _ = m.upload_scene(p)
            two = m.render_to_host(s2, 0, 8, seed=6, shard=mode)
            np.testing.assert_allclose(two, one, rtol=1e-4, atol=1e-5)
    finally:
        m.close()


# ---- 6. robustness ---------------------------------------------------------------------------------------------------------------------

def test_light_tracer_stays_in_bounds():
    """libmer_check.so: a straight (gridded sigma_t, transient film) and a curved (linear index field) light-traced scene form no index
    outside a device buffer"""
    c = capi.Context(0, check=True)
    try:
        en, *_ = c.debug_bounds()
        assert en
        yy = np.linspace(-1, 1, 5)
        rif = np.broadcast_to((RIF_A + RIF_B * yy)[None, :, None], (5, 5, 5)).astype(np.float32).copy()
        for p in (_point_scene(decomposition=P.DECOMPOSITION_TRANSIENT, min_bound=0.0, max_bound=16.0, bin_width=0.5, **_medium("grid16")),
                  _point_scene(rif_mode=P.RIF_TRILINEAR, rif=rif, stepsize=0.05, rfilter=P.FILTER_GAUSSIAN)):
            sc, vols = c.upload_scene(p, layout=capi.LAYOUT_DENSE)
            f = c.render_to_host(sc, 0, 4, seed=2)
            en, n, kind, idx, lim = c.debug_bounds()
            assert n == 0, (n, kind, idx, lim)
            assert np.isfinite(f).all() and f[..., :-2].sum() > 0
            for v in vols:
                v.destroy()
    finally:
        c.close()


def test_library_refusals(ctx):
    """what mer_render refuses for integrator = ptracer, and a collimated entry under volpath: the library's own checks (the Python
    front end's are bypassed by editing the flat scene)"""
    def desc(**kw):
        return ctx.upload_scene(_base(**kw))
    def refused(sc, msg, vols=()):
        with pytest.raises(capi.MerError, match=msg):
            ctx.render_to_host(sc, 0, 1)
    sc, _ = desc(); sc.integrator = 0
    refused(sc, "no camera path")
    sc, _ = desc(); sc.integrator = 2
    refused(sc, "unknown integrator")
    sc, _ = desc(); sc.integrator_reserved = 1
    refused(sc, "integrator_reserved")
    sc, _ = desc(); sc.env_radiance[1] = 0.5
    refused(sc, "env_radiance")
    sc, _ = desc(); sc.sensor = P.SENSOR_ORTHOGRAPHIC
    refused(sc, "perspective sensor only")
    sc, _ = desc(); sc.boundary_bsdf = P.BSDF_HDIELECTRIC
    refused(sc, "dielectric boundaries")
    sc, _ = desc(); sc.boundary = P.BOUNDARY_SDF
    refused(sc, "signed-distance")
    sc, _ = desc(); sc.point_intensity[0] = 1.0
    refused(sc, "list entries")
    sc, _ = desc(); sc.n_emitters = 0
    refused(sc, "no emitter")
    sc, _ = desc(); sc.emitters[0].type = P.EMITTER_AREA
    refused(sc, "area emitters")
    sc, _ = desc(); sc.emitters[0].type = P.EMITTER_ENVMAP
    refused(sc, "envmap")
    sc, _ = desc(); sc.emitters[0].to_world[0] = 2.0
    refused(sc, "Scale factors in the emitter-to-world transformation are not allowed!")
    sc, _ = desc(); sc.cam_to_world[0] *= 2.0; sc.cam_to_world[4] *= 2.0; sc.cam_to_world[8] *= 2.0
    refused(sc, "rigid")
    sc, _ = desc()
    with pytest.raises(capi.MerError, match="mer_render_paths"):
        ctx.render_paths(sc, 0)
    # the index field in a record layout
    sc, vols = ctx.upload_scene(_base(rif_mode=P.RIF_TRILINEAR, rif=np.ones((6, 6, 6), np.float32), stepsize=0.05), layout=capi.LAYOUT_CELL8)
    refused(sc, "dense layout")
    for v in vols:
        v.destroy()


def test_example_scene_renders():
    """host.render_xml of scenes/cfg_laser_transient.xml, both media: finite, not black, weight = the sample count"""
    path = os.path.join(ROOT, "scenes", "cfg_laser_transient.xml")
    for medium in ("homogeneous", "refractive"):
        f = host.render_xml(path, {"samples": "2", "tMin": "4", "tMax": "9", "tRes": "0.5", "medium": medium}, seed=1)
        assert f.shape == (96, 128, 10 * 3 + 2)
        assert np.isfinite(f).all() and f[..., :-2].sum() > 0 and np.all(f[..., -1] == 2)
