"""The exitance map of mer_render_exitance restated in float64 with numpy, for a grey homogeneous medium with the null boundary in the cube
[-1, 1]^3 or in a sphere about the origin (include/mer.h, mer_render_exitance, has the estimator).  Vectorised over the paths of a batch;
independent of the library.

The walk is tests/fluence64.py's (lightpath64.walk with the medium Grey; the recorder is ExitMap): emission, one depth and one roulette trip for the null boundary when the emitter lies outside,
free flights t ~ sigma_t exp(-sigma_t t) (sigma_t = 0: every flight reaches the boundary, its number drawn all the same: Grey's draw_when_clear), albedo, Henyey-Greenstein, roulette.  What is
new is what happens when a flight passes the exit of the shape: the exit point x, the direction d, the weight w = T power and the optical
path length l (exterior leg at index 1, every flight inside times the constant index n) go through the cone (c = d . normal < cos_min:
`rejected`), the window (frame = floor((l - t_min) / t_bin) outside 0 ... frames - 1: `late`) and into the cell of x.  An emitted ray that
misses the shape adds its weight to `missed` (and, as in the fluence grids, to `escaped`).

Totals (16, as mer_exitance_read): [0] paths, [1..3] escaped, [4..6] missed, [7] ended (always 0 here), [8..10] late, [11..13] rejected,
[14] exits binned, [15] 0."""
import numpy as np
from tests.lightpath64 import CUBE, Grey, ExitMap, walk, sphere, cell, point, collimated, bar, total_bar       # noqa: F401  (re-exported for the tests)


def render(emitter, sigma_s, sigma_a, g, shape, res, frames=1, t_min=0.0, t_bin=0.0, cos_min=0.0, n=1.0, paths=4096, batches=16, seed=0,
           max_depth=-1, rr_depth=5, max_events=4096, counts=False):
    """`batches` independent batches of `paths` paths: (sums (batches, frames, faces, res_v, res_u), totals (batches, 16)): raw sums as the
    library keeps them (one channel: the medium is grey; the three channels of the totals are equal).  counts = True: a third array shaped
    like sums, the number of exits binned per key"""
    rec = ExitMap(batches, 1, shape, res, frames, t_min, t_bin, cos_min, counts)
    walk(emitter, emitter["phi"], shape, Grey(sigma_s, sigma_a, draw_when_clear=True), g, [rec], n=n, paths=paths, batches=batches, seed=seed,
         max_depth=max_depth, rr_depth=rr_depth, max_events=max_events)
    out = (rec.result()[..., 0], rec.totals)
    return out + (rec.hits.reshape(out[0].shape),) if counts else out


def identity_gap(sums, totals):
    """per batch: sum(sums) + missed + rejected + late - escaped, relative to escaped"""
    lhs = sums.reshape(len(sums), -1).sum(1) + totals[:, 4] + totals[:, 11] + totals[:, 8]
    return np.abs(lhs - totals[:, 1]) / np.maximum(totals[:, 1], 1e-300)


def cube_cell_solid_angles(res):
    """solid angle of every cell of one face of the cube [-1, 1]^3 seen from the centre, (res_v, res_u): with the face at distance 1 and the
    cell [u0, u1] x [v0, v1], Omega = sum over the corners of +- atan(u v / sqrt(1 + u^2 + v^2)); the face's cells sum to 4 pi / 6"""
    ru, rv = res
    u = -1 + 2 * np.arange(ru + 1) / ru; v = -1 + 2 * np.arange(rv + 1) / rv
    U, V = np.meshgrid(u, v)                                              # (rv + 1, ru + 1)
    A = np.arctan(U * V / np.sqrt(1 + U * U + V * V))
    return A[1:, 1:] - A[1:, :-1] - A[:-1, 1:] + A[:-1, :-1]


def cell_rect(face, iv, iu, res):
    """the rectangle of a cube cell as (lo, hi) corners in 3-D"""
    axis = face // 2; ua, va = (axis + 1) % 3, (axis + 2) % 3
    lo = np.zeros(3); hi = np.zeros(3)
    lo[axis] = hi[axis] = 1.0 if face % 2 else -1.0
    lo[ua], hi[ua] = -1 + 2 * iu / res[0], -1 + 2 * (iu + 1) / res[0]
    lo[va], hi[va] = -1 + 2 * iv / res[1], -1 + 2 * (iv + 1) / res[1]
    return lo, hi
