"""The time-resolved fluence grid of mer_render_fluence (a handle of mer_fluence_time_create) restated in float64 with numpy: the walk of
tests/fluence64.py (lightpath64.walk with the medium Grey), with the path length per particle that the recorder Grid bins by (include/mer.h, mer_fluence_time_create, has the estimator).

The path length l of a deposit: the exterior leg from an emitter outside the cube to its entry point, times 1 (the index outside), plus
every free flight up to and including the one that ends at the collision, times rif_const (straight rays in a medium of constant index).
The deposit goes to frame floor((l - t_min) / t_bin) (half-open frames) of the cell that holds the point; a deposit inside the box whose
frame lies outside 0 ... frames - 1 goes to the out-of-window total, a point outside the box to `dropped` whatever its time.

Totals (12, as mer_fluence_time_read): the 8 of fluence64, then the out-of-window weight x 3, then 0."""
import numpy as np
from tests.lightpath64 import CUBE, Grey, Grid, walk, bar, total_bar          # noqa: F401  (bar and total_bar: for the tests that import this module)


def render(emitter, sigma_s, sigma_a, g, res, frames, t_min, t_bin, rif_const=1.0, bmin=(-1, -1, -1), bmax=(1, 1, 1), paths=4096, batches=16,
           seed=0, max_depth=-1, rr_depth=5, max_events=4096):
    """`batches` independent batches of `paths` paths: (sums (batches, frames, nz, ny, nx), totals (batches, 12)), raw sums as the library
    keeps them (one channel: the medium is grey; the three channels of the totals are equal)"""
    rec = Grid(batches, 1, res, bmin, bmax, frames, t_min, t_bin)
    walk(emitter, emitter["phi"], CUBE, Grey(sigma_s, sigma_a), g, [rec], n=rif_const, paths=paths, batches=batches, seed=seed, max_depth=max_depth,
         rr_depth=rr_depth, max_events=max_events)
    return rec.result()[..., 0], rec.totals


def beam_column_time(emitter, sigma_t, rif_const, res, frames, t_min, t_bin, bmin=(-1, -1, -1), bmax=(1, 1, 1)):
    """closed form for a beam along +z from outside or on the cube: per path, the probability p[f][z][y][x] that its FIRST collision falls
    into the cell during frame f.  At the depth z' behind the entry face the path length is ext + n z' (ext: the exterior leg), so frame f
    is the depth interval [(t_min + f t_bin - ext) / n, (t_min + (f + 1) t_bin - ext) / n): Beer-Lambert over its intersection with the
    cell's depth interval (an intersection thinner than 1e-12 counts as empty).  Zero off the beam's column.  Returns (p, p_late): p_late is the probability of a first collision inside the
    box but outside every frame."""
    assert emitter["kind"] == "collimated" and np.allclose(emitter["d"], [0, 0, 1])
    res = np.asarray(res); bmin = np.asarray(bmin, np.float64); bmax = np.asarray(bmax, np.float64)
    o = emitter["o"]
    assert o[2] <= -1.0, "the exterior leg ends on the entry face z = -1"
    p = np.zeros((frames, res[2], res[1], res[0]))
    if not (abs(o[0]) <= 1 and abs(o[1]) <= 1):
        return p, 0.0
    ij = np.floor((o[:2] - bmin[:2]) / (bmax[:2] - bmin[:2]) * res[:2]).astype(int)
    if np.any(ij < 0) or np.any(ij >= res[:2]):
        return p, 0.0
    ext = -1.0 - float(o[2])
    edges = bmin[2] + (bmax[2] - bmin[2]) * np.arange(res[2] + 1) / res[2]
    a = np.clip(edges[:-1], -1.0, 1.0) + 1.0; b = np.clip(edges[1:], -1.0, 1.0) + 1.0          # the cells' depth intervals
    for f in range(frames):
        fa = (t_min + f * t_bin - ext) / rif_const; fb = (t_min + (f + 1) * t_bin - ext) / rif_const
        lo = np.maximum(a, fa); hi = np.minimum(b, fb)
        on = hi - lo > 1e-12                                            # a frame edge that rounds past a cell edge it coincides with leaves no sliver
        p[f, on, ij[1], ij[0]] = np.exp(-sigma_t * lo[on]) - np.exp(-sigma_t * hi[on])
    whole = (np.exp(-sigma_t * a) - np.exp(-sigma_t * b)).sum()
    return p, whole - p.sum()
