"""The walk of the light-path kernels (mer_lightpath.hpp) restated in float64 with numpy and an RGB throughput: what tests/fluence64.py,
fluence_time64.py, fluence_track64.py and exitance64.py restate for a grey homogeneous medium, for media in which the three channels
differ.  Vectorised over the paths of a batch; independent of the library.  One walk records everything that was asked for.

Media (the cube [-1, 1]^3, null boundary):
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

The path: tests/fluence64.py's -- emitter (the geometry of fluence64.collimated / point, the power per channel given apart), one depth and
one roulette trip for the null boundary when the emitter lies outside, free flight, deposit, Henyey-Greenstein, roulette with
q = min(max_c T_c, 0.95) from depth >= rr_depth on.  T is the RGB throughput without the power.

Recorded per batch, raw sums in three channels as the library keeps them (render's docstring)."""
import numpy as np
from tests.fluence64 import _slabs, hg_sample, cells, bar, total_bar          # noqa: F401  (bar, total_bar: for the tests that import this module)
from tests.exitance64 import cell as map_cell, normal as map_normal, CUBE
from tests.fluence_track64 import _pieces, _weight

STRATEGIES = ("balance", "single", "maximum")


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


def homogeneous(sigma_s, sigma_a, strategy="balance", weight=1.0):
    ss = np.broadcast_to(np.asarray(sigma_s, np.float64), (3,)).copy(); sa = np.broadcast_to(np.asarray(sigma_a, np.float64), (3,)).copy()
    assert strategy in STRATEGIES and 0 < weight <= 1
    m = {"kind": "homogeneous", "ss": ss, "sa": sa, "st": ss + sa, "strategy": strategy, "w": float(weight)}
    if strategy == "maximum":
        m["maxexp"] = MaxExp(m["st"])
    m["rho"] = float(m["st"].min())          # `single`: the channel of the smallest sigma_t
    return m


def ramp(s_lo, s_hi, albedo):
    """albedo: one RGB triple, or a grid (nz, ny, nx, 3) of nodes spanning the cube, interpolated trilinearly (gridvolume.cpp:390-421)"""
    a = np.asarray(albedo, np.float64)
    return {"kind": "ramp", "s_lo": float(s_lo), "slope": (float(s_hi) - float(s_lo)) / 2.0,
            "albedo": a if a.ndim == 4 else np.broadcast_to(a, (3,)).copy()}


def ramp_albedo(m, p):
    """the albedo at the points p: (N, 3)"""
    a = m["albedo"]
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


def ramp_sigma(m, p):
    return m["s_lo"] + m["slope"] * (p[:, 2] + 1.0)


def _sample_homogeneous(m, rng, n):
    """sampled distances (inf: the flight does not sample the medium)"""
    u = rng.random(n)
    use = u < m["w"]
    r = np.where(use, u / m["w"], 0.0)
    if m["strategy"] == "maximum":
        t = m["maxexp"].sample(1.0 - r)
    elif m["strategy"] == "balance":
        ch = np.minimum((rng.random(n) * 3).astype(np.int64), 2)
        t = -np.log1p(-r) / m["st"][ch]
    else:
        t = -np.log1p(-r) / m["rho"]
    return np.where(use, t, np.inf)


def strategy_pdfs(m, t):
    """(transmittance (N, 3), pdfSuccess (N,), pdfFailure (N,)) at the distances t"""
    e = np.exp(-m["st"][None, :] * t[:, None])
    if m["strategy"] == "balance":
        pf = e.mean(1); ps = (m["st"][None, :] * e).mean(1)
    elif m["strategy"] == "maximum":
        pf = 1.0 - m["maxexp"].cdf(t); ps = m["maxexp"].pdf(t)
    else:
        pf = np.exp(-m["rho"] * t); ps = m["rho"] * pf
    return e, ps * m["w"], m["w"] * pf + (1.0 - m["w"])


def _sample_ramp(m, rng, x, d):
    E = -np.log1p(-rng.random(len(x)))
    a = ramp_sigma(m, x); b = m["slope"] * d[:, 2]
    disc = a * a + 2.0 * b * E
    with np.errstate(invalid="ignore", divide="ignore"):
        t = 2.0 * E / (a + np.sqrt(disc))
    return np.where(disc >= 0, t, np.inf)


def _emit(emitter, rng, N):
    if emitter["kind"] == "point":
        w = rng.random((N, 2)); z = 1 - 2 * w[:, 0]; ph = 2 * np.pi * w[:, 1]; rr = np.sqrt(np.maximum(1 - z * z, 0))
        d = np.stack([rr * np.cos(ph), rr * np.sin(ph), z], 1)
    else:
        d = np.tile(emitter["d"], (N, 1))
    return np.tile(emitter["o"], (N, 1)), d


def _add(dst, idx, w, n):
    """dst (n, 3) += the weights w (M, 3) at the keys idx (M,)"""
    for c in range(3):
        dst[:, c] += np.bincount(idx, w[:, c], n)


def render(emitter, power, medium, g, grid=None, tgrid=None, track=None, emap=None, n=1.0, paths=4096, batches=16, seed=0, max_depth=-1,
           rr_depth=5, max_events=4096):
    """`batches` independent batches of `paths` paths from `emitter` (geometry only) with the RGB `power` per path (a point emitter: 4 pi I).
    Returns a dict of raw sums, the leading axis the batch:
      grid  = dict(res, bmin, bmax): "grid" (K, nz, ny, nx, 3), "grid_totals" (K, 8): the collision grid (mer_fluence_read)
      tgrid = dict(res, frames, t_min, t_bin[, bmin, bmax]): "tgrid" (K, frames, nz, ny, nx, 3), "tgrid_totals" (K, 12) (mer_fluence_time_read)
      track = dict(res, bmin, bmax): "track" (K, nz, ny, nx, 3), "track_totals" (K, 8): the track-length grid; a homogeneous medium under
              `single` with weight 1 only (the library's analog requirement)
      emap  = dict(res=(res_u, res_v)[, frames, t_min, t_bin, cos_min]): "emap" (K, frames, 6, res_v, res_u, 3), "emap_totals" (K, 16)
              (mer_exitance_read)
      "absorbed" (K, 3): the sum over the collisions of (1 - albedo_c) T_c power_c w_c, w_c the collision's weight (1 in the ramp): the
      absorbed power, which cell sums cannot give where sigma_t varies inside a cell;  "escaped" (K, 3).
    n = the constant refractive index inside (path lengths)."""
    rng = np.random.default_rng(seed)
    power = np.broadcast_to(np.asarray(power, np.float64), (3,))
    homog = medium["kind"] == "homogeneous"
    out = {"absorbed": np.zeros((batches, 3)), "escaped": np.zeros((batches, 3))}
    tots = []
    box = lambda q: (q["res"], q.get("bmin", (-1, -1, -1)), q.get("bmax", (1, 1, 1)))
    if grid is not None:
        gn = int(np.prod(grid["res"])); gs = np.zeros((batches, gn, 3)); gt = np.zeros((batches, 8)); tots.append(gt)
    if tgrid is not None:
        tn_ = int(np.prod(tgrid["res"])); tf_ = tgrid["frames"]; ts = np.zeros((batches, tf_ * tn_, 3)); tt = np.zeros((batches, 12)); tots.append(tt)
    if track is not None:
        assert not homog or (medium["strategy"] == "single" and medium["w"] == 1.0), "the track-length weight needs analog sampling"
        kn = int(np.prod(track["res"])); ks = np.zeros((batches, kn, 3)); kt = np.zeros((batches, 8)); tots.append(kt)
        delta = medium["st"] - medium["rho"] if homog else np.zeros(3)
    if emap is not None:
        ru, rv = emap["res"]; mf = emap.get("frames", 1); mn = 6 * ru * rv
        m_tmin, m_tbin, m_cos = emap.get("t_min", 0.0), emap.get("t_bin", 0.0), emap.get("cos_min", 0.0)
        ms = np.zeros((batches, mf * mn, 3)); mt = np.zeros((batches, 16)); tots.append(mt)
    outside = not np.all(np.abs(emitter["o"]) <= 1)
    for b in range(batches):
        N = paths
        x, d = _emit(emitter, rng, N)
        T = np.ones((N, 3)); L = np.zeros(N)
        depth = 1
        esc = np.zeros(3); missed = np.zeros(3)
        if outside:                                                     # to the null boundary: one depth, one roulette trip
            tn, tf = _slabs(x, d)
            hit = (tn <= tf) & (tn > 0)
            missed += power * np.count_nonzero(~hit); esc += power * np.count_nonzero(~hit)
            x, d, T, L = x[hit] + d[hit] * tn[hit, None], d[hit], T[hit], tn[hit] * 1.0
            if depth >= rr_depth:
                q = np.minimum(T.max(1), 0.95); keep = rng.random(len(T)) < q
                x, d, T, L = x[keep], d[keep], T[keep] / q[keep, None], L[keep]
            depth += 1
        for _ in range(max_events):
            if len(T) == 0 or not (depth <= max_depth or max_depth < 0):
                break
            _, tex = _slabs(x, d)
            tfl = _sample_homogeneous(medium, rng, len(T)) if homog else _sample_ramp(medium, rng, x, d)
            sc = tfl < tex
            ex = ~sc
            # ---- the flights that reach the boundary
            we = T[ex] * power
            if homog:
                tr, _, pf = strategy_pdfs(medium, tex[ex])
                we = we * tr / pf[:, None]
            esc += we.sum(0)
            if emap is not None:
                xe = x[ex] + d[ex] * tex[ex, None]; de = d[ex]; le = L[ex] + tex[ex] * n
                cosn = (de * map_normal(xe, CUBE)).sum(1)
                rej = (cosn < m_cos) if m_cos > 0 else np.zeros(len(we), bool)
                if m_tbin > 0:
                    fr = np.floor((le - m_tmin) / m_tbin); late = ~rej & ~((fr >= 0) & (fr < mf))
                else:
                    fr = np.zeros(len(we)); late = np.zeros(len(we), bool)
                ok = ~rej & ~late
                mt[b, 11:14] += we[rej].sum(0); mt[b, 8:11] += we[late].sum(0); mt[b, 14] += np.count_nonzero(ok)
                _add(ms[b], fr[ok].astype(np.int64) * mn + map_cell(xe[ok], CUBE, (ru, rv)), we[ok], mf * mn)
            # ---- the track-length deposit of every flight, collided or not
            if track is not None:
                pa, pb, idx, inside = _pieces(x, d, np.minimum(tfl, tex), *box(track))
                wk = (T * power)[:, None, :] * (_weight(pa, pb, delta) if homog else np.repeat((pb - pa)[..., None], 3, 2))
                _add(ks[b], idx[inside], wk[inside], kn)
                kt[b, 4:7] += wk[~inside].sum(0)
            # ---- the collisions
            x, d, T, L = x[sc] + d[sc] * tfl[sc, None], d[sc], T[sc], L[sc] + tfl[sc] * n
            if len(T) == 0:
                break
            if homog:
                tr, ps, _ = strategy_pdfs(medium, tfl[sc])
                fac = tr / ps[:, None]
                wdep = T * power * fac
                out["absorbed"][b] += (medium["sa"] * wdep).sum(0)
                T = T * medium["ss"] * fac
            else:
                wdep = T * power / ramp_sigma(medium, x)[:, None]
                alb = ramp_albedo(medium, x)
                out["absorbed"][b] += ((1.0 - alb) * T * power).sum(0)
                T = T * alb
            if grid is not None:
                idx, inside = cells(x, *box(grid))
                _add(gs[b], idx[inside], wdep[inside], gn)
                gt[b, 4:7] += wdep[~inside].sum(0)
            if tgrid is not None:
                idx, inside = cells(x, *box(tgrid))
                f = np.floor((L - tgrid["t_min"]) / tgrid["t_bin"])
                timely = (f >= 0) & (f < tf_)
                mm = inside & timely
                _add(ts[b], f[mm].astype(np.int64) * tn_ + idx[mm], wdep[mm], tf_ * tn_)
                tt[b, 4:7] += wdep[~inside].sum(0); tt[b, 8:11] += wdep[inside & ~timely].sum(0)
            live = T.max(1) > 0
            x, d, T, L = x[live], d[live], T[live], L[live]
            d = hg_sample(g, d, rng.random((len(T), 2)))
            if depth >= rr_depth:
                q = np.minimum(T.max(1), 0.95); keep = rng.random(len(T)) < q
                x, d, T, L = x[keep], d[keep], T[keep] / q[keep, None], L[keep]
            depth += 1
        out["escaped"][b] = esc
        for t_ in tots:
            t_[b, 0] = N; t_[b, 1:4] = esc
        if emap is not None:
            mt[b, 4:7] = missed
    if grid is not None:
        r = grid["res"]; out["grid"] = gs.reshape((batches, r[2], r[1], r[0], 3)); out["grid_totals"] = gt
    if tgrid is not None:
        r = tgrid["res"]; out["tgrid"] = ts.reshape((batches, tf_, r[2], r[1], r[0], 3)); out["tgrid_totals"] = tt
    if track is not None:
        r = track["res"]; out["track"] = ks.reshape((batches, r[2], r[1], r[0], 3)); out["track_totals"] = kt
    if emap is not None:
        out["emap"] = ms.reshape((batches, mf, 6, rv, ru, 3)); out["emap_totals"] = mt
    return out


def ramp_column_mean(power, m, a, b):
    """per path: the closed form of an unscattered beam along +z from the face z = -1 through the ramp: both the collision
    estimator (P / sigma_t(x) at a first collision of density sigma_t exp(-tau)) and the track-length estimator have the mean
    P integral_a^b exp(-tau(s)) ds over the depth interval [a, b], tau(s) = s_lo s + slope s^2 / 2 = c^2 ((s + s0)^2 - s0^2)"""
    import math
    erf = np.vectorize(math.erf)
    c = np.sqrt(m["slope"] / 2.0); s0 = m["s_lo"] / m["slope"]
    return power * np.exp((c * s0) ** 2) * np.sqrt(np.pi) / (2 * c) * (erf(c * (b + s0)) - erf(c * (a + s0)))


def ramp_depth(m, s):
    """optical depth of the first s units behind the face z = -1 along +z"""
    return m["s_lo"] * s + m["slope"] * s * s / 2.0
