"""The fluence grid of mer_render_fluence restated in float64 with numpy, for a grey homogeneous medium in the cube [-1, 1]^3 with the null
boundary (include/mer.h, mer_render_fluence, has the estimator).  Vectorised over the paths of a batch; independent of the library.  The
event loop is tests/lightpath64.py's `walk`, with its medium Grey and its recorder Grid.

A path: emitted by a collimated beam (the fixed ray, weight = power) or a point emitter (uniform sphere, weight = 4 pi I); an emitter
outside the cube pays one depth for the null boundary (and a roulette trip); then, while depth <= max_depth (or max_depth < 0): a free
flight t ~ sigma_t exp(-sigma_t t) (medium_sampling_weight = 1), escape if it passes the exit, else a real collision: the deposit
w = T power / sigma_t into the cell that holds the point (half-open cells, floor((p - bmin) / (bmax - bmin) res); outside the box: into
`dropped`), T *= albedo, a Henyey-Greenstein direction, and the roulette: from depth >= rr_depth on the path survives with q = min(T, 0.95)
and T /= q.  T is the throughput WITHOUT the power, as the light tracer's roulette has it.

Totals (8, as mer_fluence_read): paths started, escaped weight x 3, dropped deposit weight x 3, paths ended by a budget (always 0 here)."""
import numpy as np
from tests.lightpath64 import CUBE, Grey, Grid, walk, point, collimated, bar, total_bar         # noqa: F401  (re-exported for the tests)


def render(emitter, sigma_s, sigma_a, g, res, bmin=(-1, -1, -1), bmax=(1, 1, 1), paths=4096, batches=16, seed=0, max_depth=-1, rr_depth=5,
           max_events=4096):
    """`batches` independent batches of `paths` paths: (sums (batches, nz, ny, nx), totals (batches, 8)), raw sums as the library keeps
    them (one channel: the medium is grey; the three channels of the totals are equal)"""
    rec = Grid(batches, 1, res, bmin, bmax)
    walk(emitter, emitter["phi"], CUBE, Grey(sigma_s, sigma_a), g, [rec], paths=paths, batches=batches, seed=seed, max_depth=max_depth,
         rr_depth=rr_depth, max_events=max_events)
    return rec.result()[..., 0], rec.totals


def beam_column(emitter, sigma_t, res, bmin=(-1, -1, -1), bmax=(1, 1, 1)):
    """closed form for a beam along +z: per path, the probability p[z][y][x] that its FIRST collision falls into the cell (Beer-Lambert over the
    cell's z interval clipped to the cube, counted from the entry face z = -1), zero off the beam's column.  A cell's expected sum per path
    is P / sigma_t p, its variance (P / sigma_t)^2 p (1 - p)."""
    assert emitter["kind"] == "collimated" and np.allclose(emitter["d"], [0, 0, 1])
    res = np.asarray(res); bmin = np.asarray(bmin, np.float64); bmax = np.asarray(bmax, np.float64)
    o = emitter["o"]
    p = np.zeros((res[2], res[1], res[0]))
    if not (abs(o[0]) <= 1 and abs(o[1]) <= 1):
        return p
    ij = np.floor((o[:2] - bmin[:2]) / (bmax[:2] - bmin[:2]) * res[:2]).astype(int)
    if np.any(ij < 0) or np.any(ij >= res[:2]):
        return p
    edges = bmin[2] + (bmax[2] - bmin[2]) * np.arange(res[2] + 1) / res[2]
    z0 = max(-1.0, float(o[2]))
    a = np.clip(edges[:-1], z0, 1.0) - z0; b = np.clip(edges[1:], z0, 1.0) - z0
    p[:, ij[1], ij[0]] = np.exp(-sigma_t * a) - np.exp(-sigma_t * b)
    return p
