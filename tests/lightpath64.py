"""The walk of the light-path kernels (mer_lightpath.hpp) restated in float64 with numpy: ONE event loop (`walk`) behind the seven reference
renderers -- fluence64, fluence_time64, fluence_track64, exitance64, sensitivity64, sensitivity_array64 and `render` here, which carries an
RGB throughput for media in which the three channels differ.  Vectorised over the paths of a batch; independent of the library; imports
nothing from tests/, so the other six import from here and the dependency runs one way.  A renderer = a shape, a medium, some recorders.

Shapes (null boundary): CUBE = [-1, 1]^3, or sphere(R) about the origin: _inside, _span, normal, cell.

Media (each keeps its own arithmetic: the tests compare them with one another):
* Grey(sigma_s, sigma_a): fluence64's analog medium, scalar throughput: t = -log(1 - u) / sigma_t, the deposit T power / sigma_t, T *= albedo.
* GreyRho / DeltaTracked: fluence_track64's media (a sampling density rho with a chromatic sigma_t - rho; sigma_fn below a majorant).
* homogeneous(sigma_s, sigma_a, strategy, weight): 3-vectors and a distance-sampling strategy restated from Walk::sample_exp_distance and
  strategy_pdfs (mer_walk.hpp).  A first uniform number u decides whether the flight samples the medium (u < weight; then u / weight is
  the number the distance is drawn from) or runs to the boundary.  `single`: t = -log(1 - u) / rho with rho the smallest sigma_t;
  `balance`: a second uniform number picks the channel whose sigma_t is rho; `maximum`: the density max_i sigma_i exp(-sigma_i t) / N
  through the tables of MaxExpDist as sampling_strategy (mer_scene.hip) builds them.  A collision at t weighs, per channel,
  tau_c(t) / pdfSuccess(t); a flight that reaches the boundary at d weighs tau_c(d) / pdfFailure(d) (process(), particleproc.cpp:190-196),
  tau_c = exp(-sigma_t,c t), pdfSuccess = weight x the density at t, pdfFailure = weight x P(distance > d) + (1 - weight).
* ramp(s_lo, s_hi, albedo): a grey sigma_t linear in z, s_lo at z = -1 and s_hi at z = +1, with a constant RGB albedo.  Free flights by the
  CLOSED-FORM inversion of the optical depth along the ray (no delta tracking, no majorant): with a = sigma_t at the start, b = slope d_z
  and E = -log(1 - u), a t + b t^2 / 2 = E gives t = 2 E / (a + sqrt(a^2 + 2 b E)); no collision when the discriminant is negative or t
  lies past the exit.  A deposit weighs T power / sigma_t(x), the albedo multiplies T afterwards, a path leaves with T power.
* Clear: no draw and no collision.

Recorders: Grid (collision grid, timed with frames), Track (track-length grid), ExitMap (boundary map), Balance (absorbed and escaped
sums); sensitivity64 adds the per-path matrices.  Raw sums per batch, as the library keeps them."""
import math
from types import SimpleNamespace
import numpy as np

STRATEGIES = ("balance", "single", "maximum")
CUBE = ("cube",)


# ---- emitters, shapes and the helpers every renderer shares -----------------------------------------------------------------------------------

def point(position, intensity):
    return {"kind": "point", "o": np.asarray(position, np.float64), "phi": 4.0 * np.pi * float(intensity)}


def collimated(origin, direction, power):
    d = np.asarray(direction, np.float64)
    return {"kind": "collimated", "o": np.asarray(origin, np.float64), "d": d / np.linalg.norm(d), "phi": float(power)}


def _emit(emitter, rng, N):
    """a point emitter: the uniform sphere from random((N, 2)); a collimated one draws nothing"""
    if emitter["kind"] == "point":
        w = rng.random((N, 2)); z = 1 - 2 * w[:, 0]; ph = 2 * np.pi * w[:, 1]; rr = np.sqrt(np.maximum(1 - z * z, 0))
        d = np.stack([rr * np.cos(ph), rr * np.sin(ph), z], 1)
    else:
        d = np.tile(emitter["d"], (N, 1))
    return np.tile(emitter["o"], (N, 1)), d


def sphere(radius):
    return ("sphere", float(radius))


def faces(shape):
    return 6 if shape[0] == "cube" else 1


def _slabs(x, d):
    """entry and exit parameters of the rays x + t d against the cube (float64; a zero component never divides)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / np.where(d == 0, 1e-300, d)
    a, b = (-1.0 - x) * inv, (1.0 - x) * inv
    return np.minimum(a, b).max(1), np.maximum(a, b).min(1)


def _span(x, d, shape):
    """entry and exit parameters of the rays x + t d against the shape, and whether the line meets it"""
    if shape[0] == "cube":
        tn, tf = _slabs(x, d)
        return tn, tf, tn <= tf
    R = shape[1]
    b = (x * d).sum(1); c = (x * x).sum(1) - R * R
    disc = b * b - c
    root = np.sqrt(np.maximum(disc, 0))
    return -b - root, -b + root, disc > 0


def _inside(x, shape):
    return np.all(np.abs(x) <= 1) if shape[0] == "cube" else (x * x).sum() < shape[1] ** 2


def normal(x, shape):
    """outward normal at the surface points x: cube, the axis on which |x| is largest (first on a tie), sign + when x >= 0"""
    if shape[0] == "sphere":
        return x / np.linalg.norm(x, axis=1, keepdims=True)
    axis = np.argmax(np.abs(x), 1)
    n = np.zeros_like(x)
    n[np.arange(len(x)), axis] = np.where(x[np.arange(len(x)), axis] >= 0, 1.0, -1.0)
    return n


def cell(x, shape, res):
    """flat index (face, iv, iu) of the surface points x; res = (res_u, res_v)"""
    ru, rv = res
    if shape[0] == "sphere":
        q = x / np.linalg.norm(x, axis=1, keepdims=True)
        a = np.arctan2(q[:, 1], q[:, 0]) / (2 * np.pi)
        a = np.where(a < 0, a + 1, a)
        iu = np.clip(np.floor(a * ru), 0, ru - 1).astype(np.int64)
        iv = np.clip(np.floor(0.5 * (1 + q[:, 2]) * rv), 0, rv - 1).astype(np.int64)
        return iv * ru + iu
    rows = np.arange(len(x))
    axis = np.argmax(np.abs(x), 1)
    face = 2 * axis + (x[rows, axis] >= 0)
    xu, xv = x[rows, (axis + 1) % 3], x[rows, (axis + 2) % 3]
    iu = np.clip(np.floor((xu + 1) / 2 * ru), 0, ru - 1).astype(np.int64)
    iv = np.clip(np.floor((xv + 1) / 2 * rv), 0, rv - 1).astype(np.int64)
    return (face * rv + iv) * ru + iu


def hg_sample(g, d, u):
    """a direction whose cosine mu to d has the density (1 - g^2) / (2 (1 + g^2 - 2 g mu)^1.5) (g = 0: uniform)"""
    if g == 0:
        mu = 1 - 2 * u[:, 0]
    else:
        s = (1 - g * g) / (1 - g + 2 * g * u[:, 0])
        mu = (1 + g * g - s * s) / (2 * g)
    a = np.where(np.abs(d[:, :1]) < 0.9, np.array([[1.0, 0.0, 0.0]]), np.array([[0.0, 1.0, 0.0]]))
    s1 = np.cross(a, d); s1 /= np.linalg.norm(s1, axis=1, keepdims=True); t1 = np.cross(d, s1)
    sn = np.sqrt(np.maximum(1 - mu * mu, 0)); ph = 2 * np.pi * u[:, 1]
    return s1 * (sn * np.cos(ph))[:, None] + t1 * (sn * np.sin(ph))[:, None] + d * mu[:, None]


def cells(p, res, bmin, bmax):
    """(flat index [z][y][x], inside) of the points p: half-open cells"""
    res = np.asarray(res); bmin = np.asarray(bmin, np.float64); bmax = np.asarray(bmax, np.float64)
    i = np.floor((p - bmin) / (bmax - bmin) * res).astype(np.int64)
    inside = np.all((i >= 0) & (i < res), axis=1)
    i = np.where(inside[:, None], i, 0)
    return (i[:, 2] * res[1] + i[:, 1]) * res[0] + i[:, 0], inside


def _pieces(x, d, l, res, bmin, bmax):
    """the flights x + s d, s in [0, l], cut at every plane of the grid: (a (N, M), b (N, M), flat cell (N, M), inside (N, M)); empty pieces have
    b == a"""
    res = np.asarray(res); bmin = np.asarray(bmin, np.float64); bmax = np.asarray(bmax, np.float64)
    cuts = [np.zeros((len(l), 1)), l[:, None]]
    for a in range(3):
        edges = bmin[a] + (bmax[a] - bmin[a]) * np.arange(res[a] + 1) / res[a]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (edges[None, :] - x[:, a, None]) / d[:, a, None]
        t = np.where(np.isfinite(t), t, 0.0)                               # a zero component crosses no plane of its axis
        cuts.append(np.clip(t, 0.0, l[:, None]))
    s = np.sort(np.concatenate(cuts, 1), 1)
    a_, b_ = s[:, :-1], s[:, 1:]
    b_ = np.where(b_ - a_ > 1e-12, b_, a_)                                  # two roundings of one cut: no piece, and its midpoint has no cell
    mid = 0.5 * (a_ + b_)
    pts = x[:, None, :] + d[:, None, :] * mid[:, :, None]
    idx, inside = cells(pts.reshape(-1, 3), res, bmin, bmax)
    return a_, b_, idx.reshape(a_.shape), inside.reshape(a_.shape)


def _weight(a, b, delta):
    """integral_a^b exp(-delta s) ds for every channel of delta: (..., C)"""
    a = a[..., None]; b = b[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.exp(-delta * a) * (-np.expm1(-delta * (b - a))) / delta
    return np.where(delta == 0, b - a, w)


def _add(dst, idx, w):
    """dst (n, C) += the weights w (M, C) or (M,) at the keys idx (M,)"""
    w = w[:, None] if w.ndim == 1 else w
    for c in range(dst.shape[1]):
        dst[:, c] += np.bincount(idx, w[:, c], len(dst))


def bar(mean, sd, ref, ref_var=0.0, what=""):
    """the project's bar (tests/test_gpu_ptracer.py, _bar) for `mean` (standard deviation of the mean `sd`) against `ref` (variance ref_var):
    at most 1 + 1 % of the cells beyond 4 sigma, with the floor 1e-7 max|ref| under sigma; returns z"""
    s = np.sqrt(sd * sd + ref_var)
    floor = 1e-7 * max(float(np.abs(ref).max()), 1e-30)
    z = np.abs(mean - ref) / np.maximum(s, floor)
    print("%s: %d of %d beyond 4 sigma, max z %.2f" % (what, (z > 4).sum(), z.size, z.max()))
    assert (z > 4).sum() <= 1 + 0.01 * z.size, (what, np.sort(z.ravel())[-5:])
    return z


def total_bar(totals, ref, ref_var=0.0, what=""):
    """a total over K batches against `ref`: z <= 4 (_total_bar)"""
    zt = abs(totals.mean() - ref) / np.sqrt(totals.var(ddof=1) / len(totals) + ref_var)
    print("%s: total z %.2f (mean / ref = %.5f)" % (what, zt, totals.mean() / ref))
    assert zt <= 4, (what, zt)
    return zt


# ---- media: sample(rng, x, d, tex) -> flight distances (inf: no collision); exit_weight(T, power, tex) -> the weights of the lanes that reach
# the boundary; collide(x, t, T, power) -> (deposit weights, T afterwards, absorbed weight (3,) or None).  `rgb`: the throughput is (N, 3), else
# (N,).  `delta`: sigma_t - the sampling density per channel, what the track-length deposit attenuates by.

class Medium:
    rgb = False
    delta = np.zeros(1)

    def exit_weight(self, T, power, tex):
        return T * power


class Grey(Medium):
    """fluence64's grey analog medium in its own arithmetic (no strategy_pdfs: the chromatic weights are tested against this closed form).
    draw_when_clear: at sigma_t = 0 exitance64 has always drawn the flight's number and thrown it away, which shifts every later batch of a
    point-emitter run; its seeded references depend on it, so exitance64 (alone) sets the switch."""

    def __init__(self, sigma_s, sigma_a, draw_when_clear=False):
        self.st = float(sigma_s + sigma_a); self.albedo = float(sigma_s) / self.st if self.st > 0 else 0.0
        self.draw_when_clear = draw_when_clear

    def sample(self, rng, x, d, tex):
        if self.st > 0:
            return -np.log1p(-rng.random(len(x))) / self.st
        if self.draw_when_clear:
            rng.random(len(x))
        return np.full(len(x), np.inf)

    def collide(self, x, t, T, power):
        return T * power / self.st, T * self.albedo, None


class GreyRho(Medium):
    """fluence_track64's homogeneous medium: analog flights of the density rho, a grey (or zero) albedo, sigma_t - rho per channel left to the
    track-length weight.  rho = 0 draws nothing"""

    def __init__(self, sigma_s, sigma_a, rho=None):
        st = np.atleast_1d(np.asarray(sigma_s, np.float64) + np.asarray(sigma_a, np.float64))
        assert len(st) == 1 or rho is not None, "a chromatic sigma_t needs the sampling density"
        self.rho = float(st[0]) if rho is None else float(rho)
        al = np.atleast_1d(np.asarray(sigma_s, np.float64)) / st
        assert np.all(al == al[0])
        self.albedo = float(al[0]); self.delta = st - self.rho

    def sample(self, rng, x, d, tex):
        return -np.log1p(-rng.random(len(x))) / self.rho if self.rho > 0 else np.full(len(x), np.inf)

    def collide(self, x, t, T, power):
        return None, T * self.albedo, None


class DeltaTracked(GreyRho):
    """sigma_fn(points) below the majorant sigma_max, walked with delta tracking: two draws per tentative collision, until every lane has a
    real collision or has left"""

    def __init__(self, sigma_fn, sigma_max, albedo):
        self.sigma_fn, self.sigma_max, self.albedo = sigma_fn, sigma_max, float(albedo)

    def sample(self, rng, x, d, tex):
        tfl = np.zeros(len(x)); todo = np.ones(len(x), bool)
        while todo.any():
            n = int(todo.sum())
            tfl[todo] += -np.log1p(-rng.random(n)) / self.sigma_max
            out = tfl[todo] >= tex[todo]
            real = rng.random(n) < self.sigma_fn(x[todo] + d[todo] * tfl[todo, None]) / self.sigma_max
            tfl[todo] = np.where(out, np.inf, tfl[todo])
            ix = np.flatnonzero(todo)
            todo[ix[out | real]] = False
        return tfl


class Clear(Medium):
    rgb = True
    delta = np.zeros(3)

    def sample(self, rng, x, d, tex):
        return np.full(len(x), np.inf)


class MaxExp:
    """MaxExpDist (src/medium/maxexp.h) in float64: the density max_i sigma_i exp(-sigma_i t) / N, piecewise one exponential"""

    def __init__(self, sigma_t):
        s = np.sort(np.asarray(sigma_t, np.float64))[::-1]
        assert s[0] > s[1] > s[2] > 0, "sigma_t must vary across channels"
        cdf = np.zeros(4); start = np.zeros(3)
        for i in range(3):
            lower = -1.0 if i == 0 else -(s[i] / s[i - 1]) ** (-s[i] / (s[i] - s[i - 1]))
            upper = 0.0 if i == 2 else -(s[i + 1] / s[i]) ** (-s[i] / (s[i + 1] - s[i]))
            cdf[i + 1] = cdf[i] + (upper - lower)
            start[i] = 0.0 if i == 0 else np.log(s[i] / s[i - 1]) / (s[i] - s[i - 1])
        self.s, self.start, self.norm, self.cdf_tab = s, start, cdf[3], cdf / cdf[3]

    def sample(self, u):
        i = np.clip(np.searchsorted(self.cdf_tab, u, side="left") - 1, 0, 2)
        s = self.s[i]
        return -np.log(np.exp(-self.start[i] * s) - self.norm * (u - self.cdf_tab[i])) / s

    def _interval(self, t):
        return np.clip(np.searchsorted(self.start, t, side="left") - 1, 0, 2)

    def pdf(self, t):
        s = self.s[self._interval(t)]
        return s * np.exp(-s * t) / self.norm

    def cdf(self, t):
        i = self._interval(t)
        s = self.s[i]; sp = self.s[np.maximum(i - 1, 0)]
        with np.errstate(divide="ignore", invalid="ignore"):
            lower = np.where(i == 0, -1.0, -(s / sp) ** (-s / np.where(i == 0, 1.0, s - sp)))
        return self.cdf_tab[i] + (-np.exp(-s * t) - lower) / self.norm


class homogeneous(Medium):
    rgb = True

    def __init__(self, sigma_s, sigma_a, strategy="balance", weight=1.0):
        assert strategy in STRATEGIES and 0 < weight <= 1
        self.ss = np.broadcast_to(np.asarray(sigma_s, np.float64), (3,)).copy(); self.sa = np.broadcast_to(np.asarray(sigma_a, np.float64), (3,)).copy()
        self.st = self.ss + self.sa; self.strategy = strategy; self.w = float(weight)
        self.maxexp = MaxExp(self.st) if strategy == "maximum" else None
        self.rho = float(self.st.min())          # `single`: the channel of the smallest sigma_t (sensitivity64.manual overrides it)

    delta = property(lambda self: self.st - self.rho)

    def sample(self, rng, x, d, tex):
        """sampled distances (inf: the flight does not sample the medium)"""
        n = len(x)
        u = rng.random(n)
        use = u < self.w
        r = np.where(use, u / self.w, 0.0)
        if self.strategy == "maximum":
            t = self.maxexp.sample(1.0 - r)
        elif self.strategy == "balance":
            ch = np.minimum((rng.random(n) * 3).astype(np.int64), 2)
            t = -np.log1p(-r) / self.st[ch]
        else:
            t = -np.log1p(-r) / self.rho
        return np.where(use, t, np.inf)

    def pdfs(self, t):
        """(transmittance (N, 3), pdfSuccess (N,), pdfFailure (N,)) at the distances t"""
        e = np.exp(-self.st[None, :] * t[:, None])
        if self.strategy == "balance":
            pf = e.mean(1); ps = (self.st[None, :] * e).mean(1)
        elif self.strategy == "maximum":
            pf = 1.0 - self.maxexp.cdf(t); ps = self.maxexp.pdf(t)
        else:
            pf = np.exp(-self.rho * t); ps = self.rho * pf
        return e, ps * self.w, self.w * pf + (1.0 - self.w)

    def exit_weight(self, T, power, tex):
        tr, _, pf = self.pdfs(tex)
        return T * power * tr / pf[:, None]

    def collide(self, x, t, T, power):
        tr, ps, _ = self.pdfs(t)
        fac = tr / ps[:, None]
        wdep = T * power * fac
        return wdep, T * self.ss * fac, (self.sa * wdep).sum(0)


class ramp(Medium):
    """albedo: one RGB triple, or a grid (nz, ny, nx, 3) of nodes spanning the cube, interpolated trilinearly (gridvolume.cpp:390-421)"""
    rgb = True
    delta = np.zeros(3)

    def __init__(self, s_lo, s_hi, albedo):
        a = np.asarray(albedo, np.float64)
        self.s_lo = float(s_lo); self.slope = (float(s_hi) - float(s_lo)) / 2.0
        self.albedo = a if a.ndim == 4 else np.broadcast_to(a, (3,)).copy()

    def sigma(self, p):
        return self.s_lo + self.slope * (p[:, 2] + 1.0)

    def albedo_at(self, p):
        """the albedo at the points p: (N, 3)"""
        a = self.albedo
        if a.ndim == 1:
            return np.broadcast_to(a, (len(p), 3))
        res = np.array(a.shape[2::-1])                                          # (nx, ny, nz)
        q = (p + 1.0) / 2.0 * (res - 1)
        i = np.clip(np.floor(q).astype(np.int64), 0, res - 2); f = q - i
        out = np.zeros((len(p), 3))
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    w = np.where(dx, f[:, 0], 1 - f[:, 0]) * np.where(dy, f[:, 1], 1 - f[:, 1]) * np.where(dz, f[:, 2], 1 - f[:, 2])
                    out += w[:, None] * a[i[:, 2] + dz, i[:, 1] + dy, i[:, 0] + dx]
        return out

    def sample(self, rng, x, d, tex):
        E = -np.log1p(-rng.random(len(x)))
        a = self.sigma(x); b = self.slope * d[:, 2]
        disc = a * a + 2.0 * b * E
        with np.errstate(invalid="ignore", divide="ignore"):
            t = 2.0 * E / (a + np.sqrt(disc))
        return np.where(disc >= 0, t, np.inf)

    def collide(self, x, t, T, power):
        alb = self.albedo_at(x)
        return T * power / self.sigma(x)[:, None], T * alb, ((1.0 - alb) * T * power).sum(0)


# ---- recorders: begin(b, paths), flight(b, fl), collision(b, co), end(b, paths, escaped, missed); arrays per batch --------------------------------

def exits(fl):
    """(points, directions, optical path lengths) of the lanes of a flight event that exit, worked out once for the recorders that ask"""
    if fl.out is None:
        ex = fl.ex
        fl.out = (fl.x[ex] + fl.d[ex] * fl.tex[ex, None], fl.d[ex], fl.L[ex] + fl.tex[ex] * fl.n)
    return fl.out


class Recorder:
    """totals: [0] paths, [1..3] escaped weight, as all the read-backs of the library begin"""

    def begin(self, b, paths):
        pass

    def flight(self, b, fl):
        pass

    def collision(self, b, co):
        pass

    def end(self, b, paths, escaped, missed):
        self.totals[b, 0] = paths; self.totals[b, 1:4] = escaped

    def result(self):
        return self.sums.reshape(self.shape)


class Grid(Recorder):
    """the collision grid (mer_fluence_read: totals (K, 8), [4..6] the deposits outside the box) or, with frames, the timed grid
    (mer_fluence_time_read: totals (K, 12), [8..10] the deposits inside the box but outside every frame)"""

    def __init__(self, batches, channels, res, bmin=(-1, -1, -1), bmax=(1, 1, 1), frames=None, t_min=0.0, t_bin=0.0):
        self.box, self.ncell, self.frames, self.t_min, self.t_bin = (res, bmin, bmax), int(np.prod(res)), frames, t_min, t_bin
        self.shape = (batches,) + (() if frames is None else (frames,)) + (res[2], res[1], res[0], channels)
        self.sums = np.zeros((batches, (frames or 1) * self.ncell, channels)); self.totals = np.zeros((batches, 8 if frames is None else 12))

    def collision(self, b, co):
        idx, m = cells(co.x, *self.box)
        self.totals[b, 4:7] += co.wdep[~m].sum(0)
        if self.frames is not None:
            f = np.floor((co.L - self.t_min) / self.t_bin)
            timely = (f >= 0) & (f < self.frames)
            self.totals[b, 8:11] += co.wdep[m & ~timely].sum(0)
            m = m & timely
            idx = f.astype(np.int64) * self.ncell + idx
        _add(self.sums[b], idx[m], co.wdep[m])


class Track(Recorder):
    """the track-length grid: every flight, collided or escaped, cut at the planes of the grid; totals (K, 8), [4..6] weight x length outside
    the box"""

    def __init__(self, batches, delta, res, bmin=(-1, -1, -1), bmax=(1, 1, 1)):
        self.box, self.delta, self.shape = (res, bmin, bmax), delta, (batches, res[2], res[1], res[0], len(delta))
        self.sums = np.zeros((batches, int(np.prod(res)), len(delta))); self.totals = np.zeros((batches, 8))

    def flight(self, b, fl):
        pa, pb, idx, inside = _pieces(fl.x, fl.d, np.minimum(fl.tfl, fl.tex), *self.box)
        Tp = fl.T * fl.power
        wk = (Tp[:, None, None] if Tp.ndim == 1 else Tp[:, None, :]) * (_weight(pa, pb, self.delta) if self.delta.any() else (pb - pa)[..., None])    # (N, M, C)
        ii, dropped = idx[inside], np.zeros(len(self.delta))
        for c in range(len(self.delta)):
            wc = wk[..., c]
            self.sums[b][:, c] += np.bincount(ii, wc[inside], len(self.sums[b]))
            dropped[c] = wc[~inside].sum()
        self.totals[b, 4:7] += dropped


class ExitMap(Recorder):
    """the exitance map (mer_exitance_read: totals (K, 16)): an exit goes through the cone, the window and into the cell of its point;
    counts: keep the number of exits binned per key as well"""

    def __init__(self, batches, channels, shape, res, frames=1, t_min=0.0, t_bin=0.0, cos_min=0.0, counts=False):
        self.geo, self.res, self.frames, self.t_min, self.t_bin, self.cos_min = shape, res, frames, t_min, t_bin, cos_min
        self.ncell = faces(shape) * res[0] * res[1]
        self.shape = (batches, frames, faces(shape), res[1], res[0], channels)
        self.sums = np.zeros((batches, frames * self.ncell, channels)); self.totals = np.zeros((batches, 16))
        self.hits = np.zeros((batches, frames * self.ncell, 1)) if counts else None

    def flight(self, b, fl):
        xe, de, le = exits(fl); we = fl.we; t = self.totals[b]
        rej = ((de * normal(xe, self.geo)).sum(1) < self.cos_min) if self.cos_min > 0 else np.zeros(len(we), bool)
        if self.t_bin > 0:
            fr = np.floor((le - self.t_min) / self.t_bin)
            late = ~rej & ~((fr >= 0) & (fr < self.frames))
        else:
            fr = np.zeros(len(we)); late = np.zeros(len(we), bool)
        ok = ~rej & ~late
        t[11:14] += we[rej].sum(0); t[8:11] += we[late].sum(0); t[14] += np.count_nonzero(ok)
        key = fr[ok].astype(np.int64) * self.ncell + cell(xe[ok], self.geo, self.res)
        _add(self.sums[b], key, we[ok])
        if self.hits is not None:
            self.hits[b, :, 0] += np.bincount(key, None, len(self.hits[b]))

    def end(self, b, paths, escaped, missed):
        Recorder.end(self, b, paths, escaped, missed)
        self.totals[b, 4:7] = missed


class Balance(Recorder):
    """the absorbed and the escaped weight per batch, (K, 3) each"""

    def __init__(self, batches):
        self.absorbed = np.zeros((batches, 3)); self.escaped = np.zeros((batches, 3))

    def collision(self, b, co):
        self.absorbed[b] += co.absorbed

    def end(self, b, paths, escaped, missed):
        self.escaped[b] = escaped


# ---- the walk ----------------------------------------------------------------------------------------------------------------------------------

def _take(lanes, keep):
    return tuple(a[keep] for a in lanes)


def _peak(T):
    return T if T.ndim == 1 else T.max(1)


def _roulette(rng, lanes):
    """a lane survives with q = min(max_c T_c, 0.95) and T /= q"""
    q = np.minimum(_peak(lanes[3]), 0.95); keep = rng.random(len(q)) < q
    pid, x, d, T, L = _take(lanes, keep)
    return pid, x, d, T / (q[keep] if T.ndim == 1 else q[keep, None]), L


def walk(emitter, power, shape, medium, g, recorders, n=1.0, paths=4096, batches=16, seed=0, max_depth=-1, rr_depth=5, max_events=4096):
    """`batches` x `paths` paths from `emitter` (geometry; `power` per path, scalar or RGB) through `medium` inside `shape`, every event shown
    to the `recorders`.  A lane is (path id, point x, direction d, throughput T without the power, optical path length L: the exterior leg
    at index 1, flights inside times n).  The only event loop of the seven renderers.

    THE DRAW ORDER IS THE CONTRACT: the seeded references the CPU and GPU tests were tuned on depend on it
    (tests/test_lightpath64_pins.py).
    1. Once: rng = default_rng(seed).  Then per batch:
    2. Emission: a point emitter draws random((N, 2)); a collimated emitter draws nothing.
    3. Entry, when the emitter lies outside the shape (one depth to the null boundary): if depth >= rr_depth, random(n_hit) for one roulette.
    4. Distance, per event, by the medium: Grey and GreyRho one random(n) (none at rho = 0; Grey at sigma_t = 0 only under
       draw_when_clear); homogeneous one random(n) and under `balance` a second; ramp one; DeltaTracked pairs random(m), random(m) over the
       unresolved lanes until none is left; Clear none.
    5. Scattering: after the collision update and the live filter (max_c T_c > 0), random((n, 2)) for Henyey-Greenstein.
    6. Roulette: if depth >= rr_depth, random(n).
    The loop ends on an empty batch or when depth exceeds max_depth (>= 0)."""
    rng = np.random.default_rng(seed)
    outside = not _inside(emitter["o"], shape)
    for b in range(batches):
        for r in recorders:
            r.begin(b, paths)
        x, d = _emit(emitter, rng, paths)
        lanes = (np.arange(paths), x, d, np.ones((paths, 3) if medium.rgb else paths), np.zeros(paths))
        depth = 1; n_missed = 0
        if outside:                                                     # to the null boundary: one depth, one roulette trip
            pid, x, d, T, L = lanes
            tn, _, meets = _span(x, d, shape)
            hit = meets & (tn > 0)
            n_missed = np.count_nonzero(~hit)
            lanes = (pid[hit], x[hit] + d[hit] * tn[hit, None], d[hit], T[hit], tn[hit])
            if depth >= rr_depth:
                lanes = _roulette(rng, lanes)
            depth += 1
        missed = power * n_missed; escaped = power * n_missed
        for _ in range(max_events):
            pid, x, d, T, L = lanes
            if len(T) == 0 or not (depth <= max_depth or max_depth < 0):
                break
            _, tex, _ = _span(x, d, shape)
            tfl = medium.sample(rng, x, d, tex)
            sc = tfl < tex
            ex = ~sc
            we = medium.exit_weight(T[ex], power, tex[ex])
            escaped = escaped + we.sum(0)
            fl = SimpleNamespace(pid=pid, x=x, d=d, T=T, L=L, tfl=tfl, tex=tex, ex=ex, we=we, power=power, n=n, out=None)
            for r in recorders:
                r.flight(b, fl)
            pid, x, d, T, L = pid[sc], x[sc] + d[sc] * tfl[sc, None], d[sc], T[sc], L[sc] + tfl[sc] * n
            if len(T) == 0:
                break
            wdep, T, absorbed = medium.collide(x, tfl[sc], T, power)
            live = _peak(T) > 0
            co = SimpleNamespace(pid=pid, x=x, L=L, wdep=wdep, absorbed=absorbed, live=live)
            for r in recorders:
                r.collision(b, co)
            pid, x, d, T, L = _take((pid, x, d, T, L), live)
            lanes = (pid, x, hg_sample(g, d, rng.random((len(T), 2))), T, L)
            if depth >= rr_depth:
                lanes = _roulette(rng, lanes)
            depth += 1
        for r in recorders:
            r.end(b, paths, escaped, missed)


def render(emitter, power, medium, g, grid=None, tgrid=None, track=None, emap=None, n=1.0, paths=4096, batches=16, seed=0, max_depth=-1,
           rr_depth=5, max_events=4096):
    """`batches` independent batches of `paths` paths from `emitter` (geometry only) with the RGB `power` per path (a point emitter: 4 pi I)
    through a homogeneous(...) or ramp(...) medium in the cube.  Returns a dict of raw sums, the leading axis the batch:
      grid  = dict(res, bmin, bmax): "grid" (K, nz, ny, nx, 3), "grid_totals" (K, 8): the collision grid (mer_fluence_read)
      tgrid = dict(res, frames, t_min, t_bin[, bmin, bmax]): "tgrid" (K, frames, nz, ny, nx, 3), "tgrid_totals" (K, 12) (mer_fluence_time_read)
      track = dict(res, bmin, bmax): "track" (K, nz, ny, nx, 3), "track_totals" (K, 8): the track-length grid; a homogeneous medium under
              `single` with weight 1 only (the library's analog requirement)
      emap  = dict(res=(res_u, res_v)[, frames, t_min, t_bin, cos_min]): "emap" (K, frames, 6, res_v, res_u, 3), "emap_totals" (K, 16)
              (mer_exitance_read)
      "absorbed" (K, 3): the sum over the collisions of (1 - albedo_c) T_c power_c w_c, w_c the collision's weight (1 in the ramp): the
      absorbed power, which cell sums cannot give where sigma_t varies inside a cell;  "escaped" (K, 3).
    n = the constant refractive index inside (path lengths).  The roulette: q = min(max_c T_c, 0.95) from depth >= rr_depth on."""
    power = np.broadcast_to(np.asarray(power, np.float64), (3,))
    if track is not None:
        assert not isinstance(medium, homogeneous) or (medium.strategy == "single" and medium.w == 1.0), "the track-length weight needs analog sampling"
    rec = {"balance": Balance(batches)}
    if grid is not None:
        rec["grid"] = Grid(batches, 3, **grid)
    if tgrid is not None:
        rec["tgrid"] = Grid(batches, 3, **tgrid)
    if track is not None:
        rec["track"] = Track(batches, medium.delta, **track)
    if emap is not None:
        rec["emap"] = ExitMap(batches, 3, CUBE, **emap)
    walk(emitter, power, CUBE, medium, g, list(rec.values()), n=n, paths=paths, batches=batches, seed=seed, max_depth=max_depth, rr_depth=rr_depth,
         max_events=max_events)
    out = {"absorbed": rec["balance"].absorbed, "escaped": rec["balance"].escaped}
    for key in ("grid", "tgrid", "track", "emap"):
        if key in rec:
            out[key] = rec[key].result(); out[key + "_totals"] = rec[key].totals
    return out


def ramp_column_mean(power, m, a, b):
    """per path: the closed form of an unscattered beam along +z from the face z = -1 through the ramp: both the collision
    estimator (P / sigma_t(x) at a first collision of density sigma_t exp(-tau)) and the track-length estimator have the mean
    P integral_a^b exp(-tau(s)) ds over the depth interval [a, b], tau(s) = s_lo s + slope s^2 / 2 = c^2 ((s + s0)^2 - s0^2)"""
    erf = np.vectorize(math.erf)
    c = np.sqrt(m.slope / 2.0); s0 = m.s_lo / m.slope
    return power * np.exp((c * s0) ** 2) * np.sqrt(np.pi) / (2 * c) * (erf(c * (b + s0)) - erf(c * (a + s0)))


def ramp_depth(m, s):
    """optical depth of the first s units behind the face z = -1 along +z"""
    return m.s_lo * s + m.slope * s * s / 2.0
