"""The track-length fluence grid (include/mer.h, mer_fluence_track_create) restated in float64 with numpy: the walk of tests/fluence64.py
`render` (lightpath64.walk) -- emitter, null-boundary entry, free flights, Henyey-Greenstein, roulette -- with the track-length deposit (the
recorder Track) in place of the collision deposit.  Independent of the library.

Every free flight [0, l], l = min(sampled distance, distance to the exit), is split at ALL the planes of the grid it crosses (sorted plane
parameters, the cell of each piece taken at its midpoint -- no cell-to-cell walk as on the GPU).  A piece [a, b] in cell c receives
    w = T power integral_a^b exp(-(sigma_t - rho) s) ds
per channel, rho being the density the distance was drawn with: exactly T power (b - a) where sigma_t == rho.  Pieces outside the box add
their w to `dropped`.

Media: homogeneous (lightpath64.GreyRho: sigma_s + sigma_a, scalar or one value per channel with a scalar sampling density `rho`: the `single` strategy), or a
function sigma_fn(points) below the majorant sigma_max walked with delta tracking (DeltaTracked; rho = sigma(x): w = T power (b - a)).

Totals (8, as mer_fluence_read): paths, escaped weight x 3, dropped weight x length x 3, ended (always 0)."""
import math
import numpy as np
from tests.lightpath64 import CUBE, GreyRho, DeltaTracked, Track, walk, _pieces         # noqa: F401  (_pieces: for the tests that import this module)

erf = np.vectorize(math.erf)


def render(emitter, sigma_s, sigma_a, g, res, bmin=(-1, -1, -1), bmax=(1, 1, 1), paths=4096, batches=16, seed=0, max_depth=-1, rr_depth=5,
           max_events=4096, rho=None, sigma_fn=None, sigma_max=None, albedo=None):
    """`batches` independent batches of `paths` paths: (sums (batches, nz, ny, nx[, 3]), totals (batches, 8)).  sigma_a (and sigma_s) may hold one
    value per channel when rho is given (then the sums carry a channel axis); the scattering albedo must be grey or zero."""
    medium = GreyRho(sigma_s, sigma_a, rho) if sigma_fn is None else DeltaTracked(sigma_fn, sigma_max, albedo)
    rec = Track(batches, medium.delta, res, bmin, bmax)
    walk(emitter, emitter["phi"], CUBE, medium, g, [rec], paths=paths, batches=batches, seed=seed, max_depth=max_depth, rr_depth=rr_depth,
         max_events=max_events)
    return (rec.result()[..., 0] if len(medium.delta) == 1 else rec.result()), rec.totals


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
