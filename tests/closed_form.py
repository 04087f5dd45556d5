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

    def sample_distance(self, p, o, d, maxt, seed, layout=None):
        return self.o.sample_distance(p.copy(rif_double=int(self.double)), o, d, maxt, seed)

    def eval_transmittance(self, p, o, d, maxt, seed, split=1):
        q = p.copy(rif_double=int(self.double))
        if split == 1:
            return self.o.eval_transmittance(q, o, d, maxt, seed)
        # the items in `split` chunks on as many threads, each chunk a seed of its own (an item's stream is keyed by seed and index)
        from concurrent.futures import ThreadPoolExecutor
        idx = np.array_split(np.arange(len(o)), split)
        with ThreadPoolExecutor(split) as ex:
            return np.concatenate(list(ex.map(lambda k: self.o.eval_transmittance(q, o[idx[k]], d[idx[k]], maxt[idx[k]], seed + 1000 * k), range(split))))

    def connect(self, p, p1, p2, seed, layout=None, split=1):
        q = p.copy(rif_double=int(self.double))
        if split == 1:
            return self.o.connect(q, p1, p2, seed)
        from concurrent.futures import ThreadPoolExecutor
        idx = np.array_split(np.arange(len(p1)), split)
        with ThreadPoolExecutor(split) as ex:
            return np.concatenate(list(ex.map(lambda k: self.o.connect(q, p1[idx[k]], p2[idx[k]], seed + 1000 * k), range(split))))

    def camera_rays(self, p, pos):
        return self.o.camera_rays(p, pos)

    def acoustic(self, p, pts):
        v, g, _ = self.o.rif_eval(p.copy(rif_double=int(self.double)), pts)
        return v, g

    def render(self, p, spp, seed):
        return self.o.render(p.copy(rif_double=int(self.double)), 0, spp, seed)[0]

    def renders(self, p, spp, seeds):
        return [self.render(p, spp, seed) for seed in seeds]


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

    def sample_distance(self, p, o, d, maxt, seed, layout=None):
        sc, vols = self._scene(p, layout)
        try:
            return self.c.sample_distance(sc, o, d, maxt, seed)
        finally:
            for v in vols:
                v.destroy()

    def connect(self, p, p1, p2, seed, layout=None, split=1):
        sc, vols = self._scene(p, layout)
        try:
            return self.c.connect(sc, p1, p2, seed)
        finally:
            for v in vols:
                v.destroy()

    def eval_transmittance(self, p, o, d, maxt, seed, split=1):
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

    def renders(self, p, spp, seeds):
        sc, vols = self._scene(p)
        try:
            return [self.c.render_to_host(sc, 0, spp, seed=seed) for seed in seeds]
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


# ------------------------------------------------------------------------------------ curved free flights, connections and NEE on exact rays
# n = 1.5 + 0.45 y on the trilinear grid (exact), the gridded sigma_t of scenes.curved_scene: the composed walk (delta tracking along
# trace()), the curved transmittance, mer_connect and one render against the closed-form ray of ref64.linear_index_trajectory /
# linear_index_connection and float64 quadratures of sigma_t along it.
CURVED_A, CURVED_B = 1.5, 0.45
CURVED_N = 24
CURVED_H = 0.5 * 2.0 / (CURVED_N - 1)                 # scenes.curved_scene's own step
# Verlet's path lags the exact ray by VERLET_CONST h (arc 0.6; the error grows linearly with the arc), which moves tau_exit by at most
# verlet_tau_shift(h): at this step that is below a quarter of the standard error of 200 000 walks on both rays (asserted in
# check_curved_transmittance from the closed form and the sample's own standard error, not fitted to a result)
VERLET_SMALL_H = 1e-3
CURVED_RAYS = [([-0.6, 0.5, -0.3], [1.0, 0.3, 0.2]), ([0.5, 0.2, -0.6], [-0.4, -0.3, 1.0])]
CONNECT_H = 1e-3
CONNECT_PAIRS = [([-0.5, 0.1, -0.2], [0.1, 0.6, -0.2]), ([0.4, -0.5, 0.3], [-0.3, 0.5, 0.1]), ([-0.9, 0.0, 0.0], [0.1, 0.6, -0.2])]


def curved_case(stepper=P.STEP_RK4, step=CURVED_H, **kw):
    nmin, nmax = LINEAR_FIELDS[1]
    return scenes.curved_scene(N=CURVED_N, rif=synth.linear_rif(CURVED_N, nmin, nmax), stepper=stepper, stepsize=step, **kw)


def _ray(i):
    o, d = (np.array(v, np.float64) for v in CURVED_RAYS[i])
    return o, d / np.linalg.norm(d)


def _curved_tau(p, i, **kw):
    o, d = _ray(i)
    return ref64.curve_optical_depth(CURVED_A, CURVED_B, p.density, p.density_scale, o.astype(np.float32), d.astype(np.float32), **kw)


def _verlet_lag(h, arc):
    return VERLET_CONST[CURVED_B] * h * np.asarray(arc, np.float64) / 0.6


def verlet_tau_shift(p, i, h):
    """bound on |tau_exit seen by Verlet at step h - tau_exit of the exact ray|: sigma_t looked up on the exact ray displaced by Verlet's
    lag along +-x, +-y, +-z (the three worst cases combined in quadrature: the lag has one direction), plus the lag's effect on where
    the ray leaves, sigma_t(exit) lag / |cos| to the face"""
    s, tau, sx = _curved_tau(p, i, m=20001)
    worst = []
    for ax in range(3):
        e = np.zeros(3); e[ax] = 1.0
        worst.append(max(abs(_curved_tau(p, i, m=20001, displace=lambda arc, sg=sg: sg * _verlet_lag(h, arc)[:, None] * e)[1][-1] - tau[-1])
                         for sg in (1.0, -1.0)))
    o, d = _ray(i)
    pe, ve, _ = ref64.linear_index_trajectory(CURVED_A, CURVED_B, o[None], d[None], sx * (1 - 1e-9))
    face = np.argmax(np.abs(pe[0]))
    cos = abs(ve[0, face]) / np.linalg.norm(ve[0])
    return float(np.linalg.norm(worst) + ref64.trilinear_sigma(p.density, p.density_scale, pe)[0] * _verlet_lag(h, sx) / cos)


def check_curved_transmittance(be, stepper, n=200000):
    """both estimators along two rays that bend and leave the cube: the mean of n seeded walks against exp(-tau_exit) of the exact ray"""
    h = VERLET_SMALL_H if stepper == P.STEP_VERLET else CURVED_H
    out = {}
    for i in range(len(CURVED_RAYS)):
        o, d = _ray(i)
        for est in (P.TR_RATIO, P.TR_WOODCOCK2):
            p = curved_case(stepper, h, tr_estimator=est)
            exact = np.exp(-_curved_tau(p, i)[1][-1])
            t = be.eval_transmittance(p, np.tile(o.astype(np.float32), (n, 1)), np.tile(d.astype(np.float32), (n, 1)), np.full(n, 9.0, np.float32), 3, split=8)[:, 0]
            t = t.astype(np.float64)
            se = t.std() / np.sqrt(n)
            z = (t.mean() - exact) / se
            print("curved transmittance: stepper %d ray %d estimator %d  exact %.6f  mean %.6f  se %.2e  z %+.2f" % (stepper, i, est, exact, t.mean(), se, z))
            if stepper == P.STEP_VERLET:
                shift = exact * verlet_tau_shift(p, i, h)
                print("    Verlet's path error moves the transmittance by at most %.2e = %.2f se" % (shift, shift / se))
                assert shift < 0.25 * se, (shift, se)
            assert abs(z) < 4, (stepper, i, est, t.mean(), exact, z)
            out[(i, est)] = float(z)
    return out


def _ks(t, F):
    k = np.arange(1, len(t) + 1)
    return max((k / len(t) - F).max(), (F - (k - 1) / len(t)).max())


def check_curved_free_flight(be, stepper, ray=0, layout=None, tol=4.0, n=100000):
    """n records of the composed walk from one (o, d): success rate and collision arc lengths against the free-flight law of the exact
    ray, and every record on the exact ray at its own arc length.  tol multiplies the deterministic bounds of FREE_FLIGHT_MEASURED"""
    verlet = stepper == P.STEP_VERLET
    h = VERLET_SMALL_H if verlet else CURVED_H
    p = curved_case(stepper, h)
    o, d = _ray(ray)
    o32, d32 = o.astype(np.float32), d.astype(np.float32)
    rec = be.sample_distance(p, np.tile(o32, (n, 1)), np.tile(d32, (n, 1)), np.full(n, 9.0, np.float32), 4, layout).astype(np.float64)
    s, tau, sx = _curved_tau(p, ray)
    succ = rec[:, 0] == 1
    Fmax = -np.expm1(-tau[-1])
    zs = (succ.mean() - Fmax) / np.sqrt(Fmax * (1 - Fmax) / n)
    ts = np.sort(rec[succ, 1])
    D = _ks(ts, -np.expm1(-np.interp(ts, s, tau)) / Fmax)
    print("curved free flight: stepper %d ray %d  P(collision) %.5f exact %.5f z %+.2f  KS D %.5f crit %.5f" % (stepper, ray, succ.mean(), Fmax, zs, D, _ks_crit(len(ts))))
    assert abs(zs) < 4, (succ.mean(), Fmax)
    assert D < _ks_crit(len(ts)), D
    # every record, collided or not, lies on the exact ray at its own arc length t
    t = rec[:, 1]
    rp, rv, _ = ref64.linear_index_trajectory(CURVED_A, CURVED_B, np.tile(o32.astype(np.float64), (n, 1)), np.tile(d32.astype(np.float64), (n, 1)), t)
    lag = _verlet_lag(h, t) if verlet else 0.0
    if verlet:
        print("    Verlet position error / (VERLET_CONST h t / 0.6): max %.3f" % (np.abs(rec[:, 2:5] - rp).max(1) / np.maximum(lag, 1e-12))[t > 0.05].max())
    B = {k: v * tol for k, v in FREE_FLIGHT_MEASURED[stepper].items()}
    pos = rec[:, 2:5]; mom = rec[:, 14:17]
    npos = CURVED_A + CURVED_B * pos[:, 1]
    n0 = CURVED_A + CURVED_B * float(o32[1])
    e = {"position": np.abs(pos - rp).max(1) - 1.1 * lag,                                  # Verlet: its first-order lag, 10 % above the measured constant
         "momentum": np.abs(mom - rv).max(1),                                              # dv/ds = grad n is constant: exact for either stepper
         "norm": np.abs(np.linalg.norm(mom, axis=1) - npos) - 1.1 * CURVED_B * lag,        # |d| = n(p); Verlet's p lags, so its n(p) does
         "refRatioSq": np.abs(rec[:, 13] - (npos / n0) ** 2)}
    st = ref64.trilinear_sigma(p.density, p.density_scale, pos[succ])
    e["sigmaS"] = np.abs(rec[succ, 5:8] / (np.asarray(p.albedo)[None] * st[:, None]) - 1).max(1)
    e["transmittance"] = np.abs(rec[succ, 8:11] * st[:, None] - 1).max(1)
    worst = {k: float(v.max()) for k, v in e.items()}
    print("    worst deviations " + "  ".join("%s %.2e (bound %.1e)" % (k, worst[k], B[k]) for k in worst))
    for k in worst:
        assert worst[k] < B[k], (k, worst[k], B[k])
    assert np.all(rec[:, 11] == 1) and np.all(rec[:, 12] == 1)
    # a walk that leaves reports the arc length before the step that left: one step back from the exit
    tf = rec[~succ, 1]
    slack = B["position"] + (4 * _verlet_lag(h, sx) if verlet else 0.0)
    print("    exits: t in [%.6f, %.6f], s_exit %.6f, step %.4g" % (tf.min(), tf.max(), sx, h))
    assert tf.min() > sx - h - slack and tf.max() < sx + slack, (tf.min(), tf.max(), sx)
    return worst


# check_curved_free_flight's bounds that no formula gives: the fp32 CPU oracle's worst deviation from the closed form over both rays, as
# measured (Verlet at VERLET_SMALL_H: its momentum sums up to 1700 fp32 steps; its position and |d| - n(p) stay inside the lag allowance, so
# they get the momentum's figure).  The checks allow tol times these: 4 for the oracle, 8 on the GPU (v_rcp_f32, OCML against glibc).
FREE_FLIGHT_MEASURED = {
    P.STEP_RK4: {"position": 6.0e-7, "momentum": 5.2e-7, "norm": 2.1e-7, "refRatioSq": 4.3e-7, "sigmaS": 1.6e-6, "transmittance": 1.6e-6},
    P.STEP_VERLET: {"position": 2.5e-5, "momentum": 2.5e-5, "norm": 2.5e-5, "refRatioSq": 4.3e-7, "sigmaS": 1.6e-6, "transmittance": 1.6e-6},
}


def check_linear_connection(be, layout=None, tol=4.0, n=512):
    """mer_connect on n random pairs at a small step against the exact connecting ray, and the expectation of ok x weight"""
    h = CONNECT_H
    p = curved_case(P.STEP_RK4, h)
    rng = np.random.RandomState(5)
    p1 = rng.uniform(-0.7, 0.7, (n, 3)).astype(np.float32); p2 = rng.uniform(-0.7, 0.7, (n, 3)).astype(np.float32)
    out = be.connect(p, p1, p2, 9, layout).astype(np.float64)
    ok = out[:, 0] == 1
    v0, ve, arc, opt = ref64.linear_index_connection(CURVED_A, CURVED_B, p1, p2)
    v0, ve, arc, opt = v0[ok], ve[ok], arc[ok], opt[ok]
    L = np.linalg.norm(p2.astype(np.float64) - p1, axis=1)
    assert (arc - L[ok]).max() > 0.015                                     # the pairs do bend: the arc exceeds the chord by up to 0.018
    w = out[ok, 1]
    print("connection: %.1f %% connected, weights %s" % (100 * ok.mean(), dict(zip(*np.unique(w, return_counts=True)))))
    assert 1 - ok.mean() < 0.15, ok.mean()
    B = {k: v * tol for k, v in CONNECT_MEASURED.items()}
    got = out[ok, 2:5]
    n1 = CURVED_A + CURVED_B * p1[ok, 1].astype(np.float64)
    ang = np.linalg.norm(got / np.linalg.norm(got, axis=1, keepdims=True) - v0 / n1[:, None], axis=1)
    # the solver stops at a miss distance |p(t*) - p2| < sqrt(2 tol2) = 1.41e-3, which a launch-angle error reaches at angle x |p2 - p1|;
    # its ray is Verlet's, which lags the exact one by VERLET_CONST h arc / 0.6 at p2 and is aimed off by that much to make up for it
    e = {"launch": ang * L[ok] - np.sqrt(2e-6) - _verlet_lag(h, arc),
         "norm": np.abs(np.linalg.norm(got, axis=1) - n1),
         "arrival": np.linalg.norm(out[ok, 5:8] + ve / np.linalg.norm(ve, axis=1, keepdims=True), axis=1) - (np.sqrt(2e-6) + _verlet_lag(h, arc)) / L[ok],
         "arc": np.abs(out[ok, 8] - arc), "optical": np.abs(out[ok, 9] - opt)}
    worst = {k: float(v.max()) for k, v in e.items()}
    print("    worst deviations " + "  ".join("%s %.2e (bound %.1e)" % (k, worst[k], B[k]) for k in worst))
    print("    arc - chord: closed form up to %.4f, solver up to %.4f" % ((arc - L[ok]).max(), (out[ok, 8] - L[ok]).max()))
    for k in worst:
        assert worst[k] <= B[k], (k, worst[k], B[k])
    big = arc - L[ok] > B["arc"]                                            # the arc exceeds the chord where the closed form says it does
    assert big.sum() >= 20 and np.all(out[ok, 8][big] > L[ok][big]), big.sum()
    # a failed solve restarts with probability rrweight = 0.01 and weight 1 / rrweight: the estimator keeps its expectation
    m = 200000
    p = curved_case(P.STEP_RK4, CURVED_H)
    for a_, b_ in CONNECT_PAIRS:
        o = be.connect(p, np.tile(np.array(a_, np.float32), (m, 1)), np.tile(np.array(b_, np.float32), (m, 1)), 3, layout, split=8)
        wk = np.where(o[:, 0] == 1, o[:, 1], 0.0).astype(np.float64)
        se = wk.std() / np.sqrt(m)
        print("    E[ok x weight] %s -> %s: %.4f +- %.4f (connected %.4f)" % (a_, b_, wk.mean(), se, (o[:, 0] == 1).mean()))
        assert abs(wk.mean() - 1) < 4 * se, (wk.mean(), se)
    return worst


# check_linear_connection's step terms: what the fp32 CPU oracle leaves at CONNECT_H beyond the derivable parts (measured), times tol as above
# (launch and arrival directions need none: the stopping rule and Verlet's lag cover them)
CONNECT_MEASURED = {"launch": 0.0, "norm": 2.4e-7, "arrival": 0.0, "arc": 1.8e-4, "optical": 2.3e-4}


# ------------------------------------------------------------------------------------ one render through curved NEE
CURVED_POINT = [0.6, 0.85, -0.2]           # off the camera ray (which climbs from y = 0 to 0.6), high in y: the connections bend by up to 0.24 rad


def curved_single_scatter_scene(gridded, **kw):
    base = dict(w=2, h=2, fov_x_deg=0.02, env_radiance=[0, 0, 0], point_position=CURVED_POINT, point_intensity=[1.0, 0.8, 0.5], max_depth=3,
                phase=P.PHASE_HG, g=0.5, rfilter=P.FILTER_BOX, rfilter_param=0.5)
    if not gridded:
        base.update(sigma_mode=P.SIGMA_HOMOGENEOUS, sigma_a=[0.3] * 3, sigma_s=[0.9] * 3)
    base.update(kw)
    return curved_case(**base)


def curved_single_scatter_reference(p, gridded):
    if gridded:
        return ref64.point_single_scatter_curved(CURVED_A, CURVED_B, [-1, 0, 0], [1, 0, 0], p.point_position, p.g, p.albedo[0], p.density, p.density_scale)
    return ref64.point_single_scatter_curved(CURVED_A, CURVED_B, [-1, 0, 0], [1, 0, 0], p.point_position, p.g, 0.75, sigma_t=1.2)


CURVED_SCATTER_SPP = 48000     # per batch: 4 se / ref measured 0.027 (homogeneous) and 0.039 (gridded) at 20 000 on the oracle


def check_point_single_scatter_curved(be, gridded, spp=None, batches=16):
    """exactly one scattering (max_depth = 3) of a point emitter's light, camera ray and connection both curved, HG g = 0.5 so that the
    launch direction's bend shows in the phase: the render against the float64 quadrature of the documented estimator.  `batches`
    renders of spp samples with seeds of their own give the standard error (the weight-100 restarts carry most of the variance).
    What it cannot see: a transmittance taken over the chord instead of the arc moves this radiance by +0.5 % (from the quadrature);
    the arc itself is held by check_linear_connection"""
    p = curved_single_scatter_scene(gridded)
    spp = CURVED_SCATTER_SPP if spp is None else spp
    ref, _, _, bend = curved_single_scatter_reference(p, gridded)
    got = []
    for film in be.renders(p, spp, range(100, 100 + batches)):
        got.append(film[..., :3].sum((0, 1)) / film[..., 4].sum())
    got = np.array(got, np.float64) / np.array(p.point_intensity)
    assert np.abs(got / got[:, :1] - 1).max() < 1e-5                       # grey medium: the channels differ by the intensity only
    mean, se = got[:, 0].mean(), got[:, 0].std(ddof=1) / np.sqrt(batches)
    z = (mean - ref) / se
    print("curved single scatter (%s): render %.6f +- %.6f  quadrature %.6f  z %+.2f  relative %+.4f  4 se / ref %.4f  bend up to %.3f rad"
          % ("gridded" if gridded else "homogeneous", mean, se, ref, z, mean / ref - 1, 4 * se / ref, bend.max()))
    assert 4 * se < 0.03 * ref, (se, ref)
    assert abs(z) < 4 and abs(mean / ref - 1) < 0.03, (mean, ref, z)
    return float(mean / ref - 1)
