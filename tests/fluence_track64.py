"""The track-length fluence grid (include/mer.h, mer_fluence_track_create) restated in float64 with numpy: the walk of tests/fluence64.py
`render` -- emitter, null-boundary entry, free flights, Henyey-Greenstein, roulette -- with the track-length deposit in place of the collision
deposit.  Independent of the library.

Every free flight [0, l], l = min(sampled distance, distance to the exit), is split at ALL the planes of the grid it crosses (sorted plane
parameters, the cell of each piece taken at its midpoint -- no cell-to-cell walk as on the GPU).  A piece [a, b] in cell c receives
    w = T power integral_a^b exp(-(sigma_t - rho) s) ds
per channel, rho being the density the distance was drawn with: exactly T power (b - a) where sigma_t == rho.  Pieces outside the box add
their w to `dropped`.

Media: homogeneous (sigma_s + sigma_a, scalar or one value per channel with a scalar sampling density `rho`: the `single` strategy), or a
function sigma_fn(points) below the majorant sigma_max walked with delta tracking (rho = sigma(x): w = T power (b - a)).

Totals (8, as mer_fluence_read): paths, escaped weight x 3, dropped weight x length x 3, ended (always 0)."""
import math
import numpy as np
from tests import fluence64 as F

erf = np.vectorize(math.erf)


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
    idx, inside = F.cells(pts.reshape(-1, 3), res, bmin, bmax)
    return a_, b_, idx.reshape(a_.shape), inside.reshape(a_.shape)


def _weight(a, b, delta):
    """integral_a^b exp(-delta s) ds for every channel of delta: (..., C)"""
    a = a[..., None]; b = b[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.exp(-delta * a) * (-np.expm1(-delta * (b - a))) / delta
    return np.where(delta == 0, b - a, w)


def render(emitter, sigma_s, sigma_a, g, res, bmin=(-1, -1, -1), bmax=(1, 1, 1), paths=4096, batches=16, seed=0, max_depth=-1, rr_depth=5,
           max_events=4096, rho=None, sigma_fn=None, sigma_max=None, albedo=None):
    """`batches` independent batches of `paths` paths: (sums (batches, nz, ny, nx[, 3]), totals (batches, 8)).  sigma_a (and sigma_s) may hold one
    value per channel when rho is given (then the sums carry a channel axis); the scattering albedo must be grey or zero."""
    rng = np.random.default_rng(seed)
    ncell = int(np.prod(res))
    if sigma_fn is None:
        st = np.atleast_1d(np.asarray(sigma_s, np.float64) + np.asarray(sigma_a, np.float64))
        assert len(st) == 1 or rho is not None, "a chromatic sigma_t needs the sampling density"
        rho = float(st[0]) if rho is None else float(rho)
        al = np.atleast_1d(np.asarray(sigma_s, np.float64)) / st
        assert np.all(al == al[0])
        alb = float(al[0])
        delta = st - rho
    else:
        rho = None; alb = float(albedo); delta = np.zeros(1)
    nc = len(delta)
    sums = np.zeros((batches, ncell, nc)); totals = np.zeros((batches, 8))
    outside = not np.all(np.abs(emitter["o"]) <= 1)
    for b in range(batches):
        N = paths
        totals[b, 0] = N
        if emitter["kind"] == "point":
            w = rng.random((N, 2)); z = 1 - 2 * w[:, 0]; ph = 2 * np.pi * w[:, 1]; rr = np.sqrt(np.maximum(1 - z * z, 0))
            d = np.stack([rr * np.cos(ph), rr * np.sin(ph), z], 1)
        else:
            d = np.tile(emitter["d"], (N, 1))
        x = np.tile(emitter["o"], (N, 1))
        T = np.ones(N); phi = emitter["phi"]
        depth = 1
        escaped = 0.0; dropped = np.zeros(nc)
        if outside:
            tn, tf = F._slabs(x, d)
            hit = (tn <= tf) & (tn > 0)
            escaped += phi * np.count_nonzero(~hit)
            x, d, T = x[hit] + d[hit] * tn[hit, None], d[hit], T[hit]
            if depth >= rr_depth:
                q = np.minimum(T, 0.95); keep = rng.random(len(T)) < q
                x, d, T = x[keep], d[keep], T[keep] / q[keep]
            depth += 1
        for _ in range(max_events):
            if len(T) == 0 or not (depth <= max_depth or max_depth < 0):
                break
            _, tex = F._slabs(x, d)
            if sigma_fn is None:
                tfl = -np.log1p(-rng.random(len(T))) / rho if rho > 0 else np.full(len(T), np.inf)
            else:                                                           # delta tracking below the majorant
                tfl = np.zeros(len(T)); todo = np.ones(len(T), bool)
                while todo.any():
                    n = int(todo.sum())
                    tfl[todo] += -np.log1p(-rng.random(n)) / sigma_max
                    out = tfl[todo] >= tex[todo]
                    real = rng.random(n) < sigma_fn(x[todo] + d[todo] * tfl[todo, None]) / sigma_max
                    tfl[todo] = np.where(out, np.inf, tfl[todo])
                    ix = np.flatnonzero(todo)
                    todo[ix[out | real]] = False
            sc = tfl < tex
            # ---- the track-length deposit of every flight, collided or escaped
            l = np.minimum(tfl, tex)
            pa, pb, idx, inside = _pieces(x, d, l, res, bmin, bmax)
            wdep = (T * phi)[:, None, None] * _weight(pa, pb, delta)         # (N, M, C)
            for c in range(nc):
                sums[b, :, c] += np.bincount(idx[inside], wdep[..., c][inside], ncell)
                dropped[c] += wdep[..., c][~inside].sum()
            escaped += phi * T[~sc].sum()
            x, d, T = x[sc] + d[sc] * tfl[sc, None], d[sc], T[sc]
            if len(T) == 0:
                break
            T = T * alb
            live = T > 0
            x, d, T = x[live], d[live], T[live]
            d = F.hg_sample(g, d, rng.random((len(T), 2)))
            if depth >= rr_depth:
                q = np.minimum(T, 0.95); keep = rng.random(len(T)) < q
                x, d, T = x[keep], d[keep], T[keep] / q[keep]
            depth += 1
        totals[b, 1:4] = escaped
        totals[b, 4:7] = dropped if nc == 3 else dropped[0]
    shape = (batches, res[2], res[1], res[0])
    return (sums[..., 0].reshape(shape) if nc == 1 else sums.reshape(shape + (3,))), totals


def column_depths(emitter, res, bmin=(-1, -1, -1), bmax=(1, 1, 1)):
    """the column of a beam along +z: (on (nz, ny, nx) bool, a (nz,), b (nz,)): the depth interval [a_k, b_k] of the cells of slab k, from the
    entry face z = -1 on, clipped to the cube (fluence64.beam_column's geometry)"""
    assert emitter["kind"] == "collimated" and np.allclose(emitter["d"], [0, 0, 1])
    res = np.asarray(res); bmin = np.asarray(bmin, np.float64); bmax = np.asarray(bmax, np.float64)
    o = emitter["o"]
    on = np.zeros((res[2], res[1], res[0]), bool)
    ij = np.floor((o[:2] - bmin[:2]) / (bmax[:2] - bmin[:2]) * res[:2]).astype(int)
    edges = bmin[2] + (bmax[2] - bmin[2]) * np.arange(res[2] + 1) / res[2]
    z0 = max(-1.0, float(o[2]))
    a = np.clip(edges[:-1], z0, 1.0) - z0; b = np.clip(edges[1:], z0, 1.0) - z0
    if abs(o[0]) <= 1 and abs(o[1]) <= 1 and np.all(ij >= 0) and np.all(ij < res[:2]):
        on[b > a, ij[1], ij[0]] = True
    return on, a, b


def absorber_moments(power, sigma, a, b):
    """a pure absorber sampled analogously (rho = sigma): per path, the mean and the second moment of the deposit P (min(t, b) - a)+ of a column
    cell with the depth interval [a, b], t ~ sigma exp(-sigma t)"""
    dl = b - a
    mean = power * np.exp(-sigma * a) * (-np.expm1(-sigma * dl)) / sigma
    second = power ** 2 * np.exp(-sigma * a) * 2 * ((-np.expm1(-sigma * dl)) / sigma ** 2 - dl * np.exp(-sigma * dl) / sigma)
    return mean, second


def beer_mean(power, sigma, a, b):
    """per path: P (e^{-sigma a} - e^{-sigma b}) / sigma, the fluence integral of an unscattered beam over [a, b] whatever the sampling density"""
    return power * (np.exp(-sigma * a) - np.exp(-sigma * b)) / sigma


def ramp_mean(power, c, a, b):
    """per path: P sqrt(pi) / (2 c) (erf(c b) - erf(c a)): the beam through sigma_t(s) = 2 c^2 s, transmittance exp(-(c s)^2)"""
    return power * np.sqrt(np.pi) / (2 * c) * (erf(c * b) - erf(c * a))
