"""Checks of the leaf operations against the float64 closed forms of tests/ref64.py, written once for two backends: the CPU oracle
(tests/test_ref64.py) and the HIP kernels (tests/test_gpu_closed_form.py).  Each check returns the largest error it saw."""
import numpy as np
from mitsubaer_amd import params as P, synth
from tests import ref64, scenes

# Verlet (heterogeneousrefractive.cpp:653-661, er_step: p += h v / n with n at the start of the step, opt += h n) is first order:
# max |p - p*| / h over 64 rays and arc length 0.6 in n = a + b y, measured with the oracle (fp32 and fp64 alike) at h = 0.075.
VERLET_CONST = {0.15: 0.0303, 0.45: 0.0921}
VERLET_OPT_CONST = {0.15: 0.0451, 0.45: 0.141}
LINEAR_FIELDS = [(1.3, 1.6), (1.05, 1.95)]          # synth.linear_rif's slope (a = 1.45, b = 0.15) and a steeper one (a = 1.5, b = 0.45)


class Oracle:
    def __init__(self, orc, double=False):
        self.o, self.double = orc, double

    def er_trace(self, p, p0, d0, dist, layout=None):
        return self.o.er_trace(p.copy(rif_double=int(self.double)), p0, d0, dist)

    def sample_distance(self, p, o, d, maxt, seed):
        return self.o.sample_distance(p, o, d, maxt, seed)

    def eval_transmittance(self, p, o, d, maxt, seed):
        return self.o.eval_transmittance(p, o, d, maxt, seed)

    def camera_rays(self, p, pos):
        return self.o.camera_rays(p, pos)

    def acoustic(self, p, pts):
        v, g, _ = self.o.rif_eval(p.copy(rif_double=int(self.double)), pts)
        return v, g

    def render(self, p, spp, seed):
        return self.o.render(p, 0, spp, seed)[0]


class Gpu:
    def __init__(self, ctx):
        self.c = ctx

    def _scene(self, p, layout=None):
        from mitsubaer_amd import capi
        return self.c.upload_scene(p, layout=capi.LAYOUT_DENSE if layout is None else layout)

    def er_trace(self, p, p0, d0, dist, layout=None):
        sc, vols = self._scene(p, layout)
        try:
            return self.c.er_trace(sc, p0, d0, dist)
        finally:
            for v in vols:
                v.destroy()

    def sample_distance(self, p, o, d, maxt, seed):
        sc, vols = self._scene(p)
        try:
            return self.c.sample_distance(sc, o, d, maxt, seed)
        finally:
            for v in vols:
                v.destroy()

    def eval_transmittance(self, p, o, d, maxt, seed):
        sc, vols = self._scene(p)
        try:
            return self.c.eval_transmittance(sc, o, d, maxt, seed)
        finally:
            for v in vols:
                v.destroy()

    def camera_rays(self, p, pos):
        sc, vols = self._scene(p)
        try:
            return self.c.camera_rays(sc, pos)
        finally:
            for v in vols:
                v.destroy()

    def acoustic(self, p, pts):
        sc, vols = self._scene(p)
        try:
            return self.c.acoustic_value_grad(sc, pts)
        finally:
            for v in vols:
                v.destroy()

    def render(self, p, spp, seed):
        sc, vols = self._scene(p)
        try:
            return self.c.render_to_host(sc, 0, spp, seed=seed)
        finally:
            for v in vols:
                v.destroy()


# ------------------------------------------------------------------------------------ eikonal trace in a linear index
def linear_scene(nmin, nmax, stepper, h, kind="trilinear"):
    """n = a + b y over the medium [-1,1]^3: a trilinear grid reproduces it exactly; the B-spline grid extends 0.8 past the medium on
    every side (8 strides: the mirror boundary's error, which decays as (2 - sqrt 3)^k, is below 1e-6 of the slope there)"""
    if kind == "trilinear":
        return scenes.curved_scene(N=24, rif=synth.linear_rif(24, nmin, nmax), stepper=stepper, stepsize=h)
    N = 37
    b = (nmax - nmin) / 2
    ax = np.linspace(-1.8, 1.8, N)
    rif = np.ascontiguousarray(np.broadcast_to((nmin + b + b * ax)[None, :, None], (N, N, N))).astype(np.float32)
    return scenes.bspline_scene(N=24, stepper=stepper, stepsize=h).copy(rif=rif, rif_aabb=([-1.8] * 3, [1.8] * 3))


def check_linear_trace(be, nmin, nmax, stepper, kind="trilinear", layout=None, hs=(0.3, 0.15, 0.075), tol=2e-6):
    a, b = (nmin + nmax) / 2, (nmax - nmin) / 2
    n = 64
    p0 = scenes.rand_points(n, -0.3, 0.3, seed=11); d0 = scenes.rand_dirs(n, seed=12)
    s = 0.6
    rp, rv, ro = ref64.linear_index_trajectory(a, b, p0, d0, s)
    ep, eo = [], []
    worst = 0.0
    for h in hs:
        op, ov, ds, oo, ok = be.er_trace(linear_scene(nmin, nmax, stepper, h, kind), p0, d0, np.full(n, s, np.float32), layout)
        assert ok.all()
        assert np.abs(ds - s).max() < 1e-6
        # dv/ds = grad n is constant: v(s) = v0 + s b e_y exactly, for either stepper
        vtol = 2e-5 if stepper == P.STEP_VERLET else tol
        assert np.abs(ov - rv).max() < vtol, np.abs(ov - rv).max()
        if stepper == P.STEP_RK4:                      # |v| = n(p) (Verlet's p lags: its n(p) carries the position error)
            assert np.abs(np.linalg.norm(ov, axis=1) - (a + b * op[:, 1].astype(np.float64))).max() < tol
        ep.append(np.abs(op - rp).max()); eo.append(np.abs(oo - ro).max())
        if stepper == P.STEP_RK4:                      # classic RK4 reaches float32 round-off on a linear field at every step size
            assert ep[-1] < tol and eo[-1] < tol, (h, ep[-1], eo[-1])
            worst = max(worst, ep[-1], eo[-1], np.abs(ov - rv).max())
        else:
            assert abs(ep[-1] / h / VERLET_CONST[round(b, 2)] - 1) < 0.1, (h, ep[-1] / h)
            assert abs(eo[-1] / h / VERLET_OPT_CONST[round(b, 2)] - 1) < 0.1, (h, eo[-1] / h)
            worst = max(worst, abs(ep[-1] / h / VERLET_CONST[round(b, 2)] - 1))
    if stepper == P.STEP_VERLET:
        for i in range(len(hs) - 1):
            order = np.log(ep[i] / ep[i + 1]) / np.log(hs[i] / hs[i + 1])
            assert abs(order - 1) < 0.1, (hs[i], order)
            order = np.log(eo[i] / eo[i + 1]) / np.log(hs[i] / hs[i + 1])
            assert abs(order - 1) < 0.1, (hs[i], order)
    return worst


def check_bouguer(be, stepper=P.STEP_RK4):
    """radial index n = 2 - r^2/3: |r x v| is conserved along the ray (the trilinear grid's error included)"""
    p = scenes.curved_scene(N=48, rif="radial", stepper=stepper, stepsize=2e-3)
    n = 256
    p0 = scenes.rand_points(n, -0.4, 0.4); d0 = scenes.rand_dirs(n)
    op, ov, ds, oo, ok = be.er_trace(p, p0, d0, np.full(n, 0.5, np.float32))
    assert ok.all()
    r0 = np.linalg.norm(p0.astype(np.float64), axis=1) ** 2
    L0 = np.cross(p0, d0 * (2 - r0 / 3)[:, None]); L1 = np.cross(op.astype(np.float64), ov)
    err = np.abs(L1 - L0).max()
    assert err < 3e-3, err
    return err


# ------------------------------------------------------------------------------------ acoustic RIF
AC = dict(n_o=float(np.float32(1.3333)), n_max=float(np.float32(0.05)), k_r=6.0)


def acoustic_points(m, k_r, seed=0):
    """random points, points on the axis and within the 1e-8 clamp, and points at r within 1e-3 of the first two zeros of J_m"""
    rng = np.random.RandomState(seed + m)
    pts = rng.uniform(-0.9, 0.9, (2000, 3))
    ax = np.array([[0.1, 0, 0], [0.3, 1e-9, 0], [-0.2, 0, -5e-9], [0.0, 3e-9, 3e-9], [0.4, 7e-9, -2e-9]])
    # zeros of J_m by bisection of the trapezoid reference on a bracket grid
    x = np.linspace(0.5, 12, 2000); j = ref64.bessel_j(m, x)
    zs = []
    for i in np.nonzero(np.sign(j[1:]) != np.sign(j[:-1]))[0][:2]:
        lo, hi = x[i], x[i + 1]
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            if np.sign(ref64.bessel_j(m, mid)) == np.sign(ref64.bessel_j(m, lo)):
                lo = mid
            else:
                hi = mid
        zs.append(0.5 * (lo + hi))
    r = np.concatenate([[z / k_r + e for e in (-1e-3, -1e-5, 0.0, 1e-5, 1e-3)] for z in zs])
    ang = rng.uniform(-np.pi, np.pi, len(r))
    near = np.stack([rng.uniform(-0.5, 0.5, len(r)), r * np.sin(ang), r * np.cos(ang)], 1)
    return np.concatenate([pts, ax, near]).astype(np.float32)


def check_acoustic(be, m, atol):
    """value and gradient against the float64 Bessel reference; atol is in units of n_max (the field's own scale)"""
    p = scenes.homogeneous_scene(rif_mode=P.RIF_ACOUSTIC, ac_n_o=AC["n_o"], ac_n_max=AC["n_max"], ac_k_r=AC["k_r"], ac_mode=m, stepsize=0.01)
    pts = acoustic_points(m, AC["k_r"])
    v, g = be.acoustic(p, pts)
    rv, rg = ref64.acoustic_value_grad(AC["n_o"], AC["n_max"], AC["k_r"], m, pts.astype(np.float64))
    ev = np.abs(v - rv).max() / AC["n_max"]
    eg = (np.abs(g - rg) / (AC["n_max"] * AC["k_r"])).max()
    assert ev < atol and eg < atol, (ev, eg)
    assert np.all(g[:, 0] == 0)
    return max(ev, eg)


# ------------------------------------------------------------------------------------ transmittance and free flight
def ramp_scene(**kw):
    """sigma_t(x) = 4 (0.5 + 0.25 x) on [-1,1]^3: linear along x, so exactly linear along any ray parallel to x"""
    N = 33
    ramp = np.broadcast_to((0.5 + 0.25 * np.linspace(-1, 1, N, dtype=np.float32))[None, None, :], (N, N, N)).copy()
    p = scenes.straight_scene(N=8, **kw)
    p.density = ramp
    return p


def _ks_crit(n, alpha_coef=1.95):
    """Kolmogorov-Smirnov critical value, alpha = 1e-3 (c = 1.95)"""
    return alpha_coef / np.sqrt(n)


def check_transmittance(be):
    errs = {}
    # Simpson quadrature is exact on a density that is linear along the ray
    p = ramp_scene(method=P.METHOD_SIMPSON)
    o = np.array([[-0.5, 0.1, -0.2], [-0.9, 0.3, 0.4], [-2.0, 0.0, 0.0], [0.2, -0.6, 0.7]], np.float32)
    d = np.array([[1, 0, 0], [1, 0, 0], [1, 0, 0], [-1, 0, 0]], np.float32)
    maxt = np.array([1.0, 1.5, 2.95, 1.1], np.float32)
    tr = be.eval_transmittance(p, o, d, maxt, 3)[:, 0]
    sig = lambda x: 4 * (0.5 + 0.25 * x)
    exact = []
    for i in range(4):
        x0, x1 = sorted([max(-1.0, min(1.0, float(o[i, 0]))), max(-1.0, min(1.0, float(o[i, 0] + d[i, 0] * maxt[i])))])
        exact.append(ref64.linear_sigma_transmittance(sig(x0), 1.0, x1 - x0))
    np.testing.assert_allclose(tr, exact, rtol=2e-6)
    errs["simpson"] = float(np.abs(tr / exact - 1).max())
    # ratio tracking and Woodcock-2 are unbiased for exp(-int sigma_t)
    n = 400000
    o = np.tile(np.array([[-0.5, 0.1, -0.2]], np.float32), (n, 1)); d = np.tile(np.array([[1, 0, 0]], np.float32), (n, 1))
    exact = ref64.linear_sigma_transmittance(sig(-0.5), 1.0, 1.0)
    for est in (P.TR_RATIO, P.TR_WOODCOCK2):
        t = be.eval_transmittance(ramp_scene(tr_estimator=est), o, d, np.full(n, 1.0, np.float32), 3)[:, 0].astype(np.float64)
        z = abs(t.mean() - exact) / (t.std() / np.sqrt(n))
        assert z < 4, (est, t.mean(), exact)
        errs["est%d_sigma" % est] = float(z)
    # delta-tracking collision distances: KS against the closed-form free-flight CDF, conditioned on a collision before maxt
    n = 100000
    o = np.tile(np.array([[-0.9, 0.05, 0.1]], np.float32), (n, 1)); d = np.tile(np.array([[1, 0, 0]], np.float32), (n, 1))
    L = 1.5
    rec = be.sample_distance(ramp_scene(), o, d, np.full(n, L, np.float32), 4)
    succ = rec[:, 0] == 1
    Fmax = ref64.linear_sigma_free_flight_cdf(sig(-0.9), 1.0, L)
    assert abs(succ.mean() - Fmax) < 4 * np.sqrt(Fmax * (1 - Fmax) / n)
    t = np.sort(rec[succ, 1].astype(np.float64))
    F = ref64.linear_sigma_free_flight_cdf(sig(-0.9), 1.0, t) / Fmax
    k = np.arange(1, len(t) + 1)
    D = max((k / len(t) - F).max(), (F - (k - 1) / len(t)).max())
    assert D < _ks_crit(len(t)), D
    errs["ks_D_over_crit"] = float(D / _ks_crit(len(t)))
    # heterogeneousrefractive sampleDistance limits: constant sigma_t = 2 through the curved estimator along +y (a straight ray,
    # n = 1.45 + 0.15 y), exit after 1.2 => P(success) = 1 - e^{-2.4}; refRatioSq = n_end^2 / n_start^2 (heterogeneousrefractive.cpp:469,501)
    p = scenes.curved_scene(N=24, sigma_mode=P.SIGMA_HOMOGENEOUS, strategy=P.STRATEGY_SINGLE, channel=0,
                            medium_sampling_weight=1.0, sigma_a=[0.2] * 3, sigma_s=[1.8] * 3, stepper=P.STEP_VERLET)
    n = 20000
    o = np.tile(np.array([[0, -0.2, 0]], np.float32), (n, 1)); d = np.tile(np.array([[0, 1, 0]], np.float32), (n, 1))
    rec = be.sample_distance(p, o, d, np.full(n, 9.0, np.float32), 2)
    succ = rec[:, 0] == 1
    ps = -np.expm1(-2.4)
    assert abs(succ.mean() - ps) < 4 * np.sqrt(ps * (1 - ps) / n)
    t = np.sort(rec[succ, 1].astype(np.float64)); F = -np.expm1(-2 * t) / ps; k = np.arange(1, len(t) + 1)
    D = max((k / len(t) - F).max(), (F - (k - 1) / len(t)).max())
    assert D < _ks_crit(len(t)) + 2 * p.stepsize, D                                  # distances quantised by the step
    ny = 1.45 + 0.15 * rec[:, 3].astype(np.float64)
    np.testing.assert_allclose(rec[:, 13], (ny / 1.42) ** 2, rtol=2e-3)
    np.testing.assert_allclose(np.linalg.norm(rec[:, 14:17], axis=1), ny, rtol=2e-3)
    return errs


# ------------------------------------------------------------------------------------ camera
CAMERAS = [(48, 40, 95.8402), (64, 16, 10.0), (17, 33, 150.0), (40, 40, 2.0)]


def check_camera(be, w, h, fov):
    c2w = P.look_at([-3, 0.2, 0.1], [-2, 0.1, 0.3], [0, 1, 0])
    p = scenes.straight_scene(N=8, w=w, h=h, fov_x_deg=fov, cam_to_world=c2w)
    xs = np.concatenate([np.arange(w + 1), np.arange(w) + 0.5]); ys = np.concatenate([np.arange(h + 1), np.arange(h) + 0.5])
    X, Y = np.meshgrid(xs, ys)
    pos = np.stack([X.ravel(), Y.ravel()], 1).astype(np.float32)          # every pixel corner and centre
    o, d = be.camera_rays(p, pos)
    ro, rd = ref64.pinhole_rays(c2w, w, h, fov, pos)
    eo, ed = np.abs(o - ro).max(), np.abs(d - rd).max()
    assert eo < 1e-6 and ed < 1e-6, (eo, ed)
    return max(eo, ed)


# ------------------------------------------------------------------------------------ render-level known answers
def check_emission_slab(be, spp=256):
    """emissive, non-scattering medium, no light from outside: L = eps (1 - exp(-sigma_t chord)) per pixel, the chord of the pixel's
    own camera ray through the cube (collision estimator, box filter of radius half a pixel)"""
    w = h = 16
    p = scenes.straight_scene(N=8, w=w, h=h, albedo=[0, 0, 0], env_radiance=[0, 0, 0], emission=[1.0, 0.6, 0.3],
                              rfilter=P.FILTER_BOX, rfilter_param=0.5, fov_x_deg=30.0)
    p.density = np.full((8, 8, 8), 0.5, np.float32)
    film = be.render(p, spp, 2)
    img = film[..., :3] / film[..., 4:5]
    # the pixel's radiance is its mean over the pixel footprint: 8 x 8 sub-samples of the closed form
    sub = (np.arange(8) + 0.5) / 8
    Y, X, B, A = np.meshgrid(np.arange(h), np.arange(w), sub, sub, indexing="ij")
    pos = np.stack([(X + A).ravel(), (Y + B).ravel()], 1)
    o, d = ref64.pinhole_rays(p.cam_to_world, w, h, p.fov_x_deg, pos)
    chord = ref64.box_chord(o, d, [-1] * 3, [1] * 3).reshape(h, w, 64)
    expect = (1 - np.exp(-2.0 * chord)).mean(2)[..., None] * np.array([1.0, 0.6, 0.3])
    err = np.abs(img.mean((0, 1)) - expect.mean((0, 1))).max()
    assert err < 1e-2, err
    per_pixel = np.abs(img - expect).max()
    assert per_pixel < 0.12, per_pixel
    return err


def single_scatter_scene(**kw):
    base = dict(w=2, h=2, fov_x_deg=0.02, sigma_a=[0.3] * 3, sigma_s=[0.9] * 3, env_radiance=[0, 0, 0], point_position=[0.1, 0.6, -0.2],
                point_intensity=[1.0, 0.8, 0.5], max_depth=3, rfilter=P.FILTER_BOX, rfilter_param=0.5)
    base.update(kw)
    return scenes.homogeneous_scene(**base)


def check_point_single_scatter(be, spp=60000):
    """point emitter, homogeneous isotropic medium, exactly one scattering event (max_depth = 3: the null boundary crossing counts as a
    depth): the radiance along the central camera ray against the float64 quadrature"""
    p = single_scatter_scene()
    film = be.render(p, spp, 11)
    got = film[..., :3].sum((0, 1)) / film[..., 4].sum()
    ref, _, _, _ = ref64.point_single_scatter([-3, 0, 0], [1, 0, 0], 2.0, 4.0, 0.3, 0.9, p.point_position)
    err = np.abs(got / (ref * np.array(p.point_intensity)) - 1).max()
    assert err < 0.03, (got, ref)
    return err


def check_point_single_scatter_transient(be, spp=120000):
    """the same, time resolved: a path scattering at depth t has optical length 2 + t + d(t) (camera edge 2, n = 1)"""
    frames = 16
    p = single_scatter_scene(decomposition=P.DECOMPOSITION_TRANSIENT, min_bound=2.0, max_bound=6.0, bin_width=0.25)
    film = be.render(p, spp, 11)
    got = film[..., :-2].reshape(2, 2, frames, 3).sum((0, 1)) / film[..., -1].sum()
    _, t, f, r = ref64.point_single_scatter([-3, 0, 0], [1, 0, 0], 2.0, 4.0, 0.3, 0.9, p.point_position, n=400000)
    bins = np.floor((t + r - 2.0) / 0.25).astype(int)              # t from the camera: optical length t + r, frames from 2
    keep = (bins >= 0) & (bins < frames)
    ref = np.bincount(bins[keep], weights=f[keep], minlength=frames)
    assert ref[:2].sum() == 0 and got[:2].sum() == 0
    big = ref > 0.02 * ref.max()
    err = np.abs(got[big, 0] / ref[big] - 1).max()
    assert err < 0.06, err
    np.testing.assert_allclose(got.sum(0), ref.sum() * np.array(p.point_intensity), rtol=0.03)
    return err


def check_point_curved_equals_straight(be, spp=3000):
    """the curved branch (connection solver + transmittance along the connecting ray) reproduces the straight branch in a constant index 1"""
    N = 12
    kw = dict(w=4, h=4, env_radiance=[0, 0, 0], point_position=[0.2, 0.3, -0.1], point_intensity=[1.0, 0.8, 0.5], max_depth=3,
              rfilter=P.FILTER_BOX, rfilter_param=0.5)
    fs = be.render(scenes.straight_scene(N=N, **kw), spp, 2)
    fc = be.render(scenes.curved_scene(N=N, rif=np.ones((N, N, N), np.float32), **kw), spp, 2)
    a = fs[..., :3].sum((0, 1)) / fs[..., 4].sum(); b = fc[..., :3].sum((0, 1)) / fc[..., 4].sum()
    assert a.min() > 0
    np.testing.assert_allclose(b, a, rtol=0.08)
    return float(np.abs(b / a - 1).max())
