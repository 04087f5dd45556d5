"""The sensitivity grid of mer_render_sensitivity (include/mer.h) restated in float64 with numpy, for a homogeneous RGB medium or the
sigma_t ramp of tests/lightpath64.py (ramp(...): a constant RGB albedo or an albedo grid) with the null boundary in the cube [-1, 1]^3.
Vectorised over the paths of a batch; independent of the library.

The walk is tests/lightpath64.py's (render): emitter, one depth and one roulette trip for the null boundary when the emitter lies outside,
free flights by the medium's distance-sampling strategy, the weights transmittance / pdfSuccess at a collision and transmittance /
pdfFailure at the exit, Henyey-Greenstein, roulette.  `manual(...)` adds the strategy the derivative test needs: one exponential of a
FIXED density rho, whatever sigma_t is (Walk::sample_exp_distance with MER_STRATEGY_MANUAL), so that the walks at two values of sigma_a
draw the same paths.  In a ramp the free flights come from lightpath64._sample_ramp (the closed-form inversion of the optical depth), a
collision multiplies T by lightpath64.ramp_albedo at its point, and a path leaves with T power and no strategy factor.

What is new: nothing is deposited while a path walks.  Every flight is cut at the planes of the grid (fluence_track64._pieces) and the
lengths of its pieces are added to the path's own row of a dense matrix L[path, cell] (the grids here are small).  A path that leaves
goes through the detector in the expressions of exitance64 -- the cone (cos_min > 0 and d . normal < cos_min: rejected), the gate
(t_bin > 0: detected iff floor((l - t_min) / t_bin) == 0) and the window (the exit's cell lies on `face`, iu0 <= iu < iu1, iv0 <= iv < iv1)
-- and, detected, keeps its weight w.  After the walk J = w^T L over the detected paths.

Totals (16, as mer_sensitivity_read): [0] paths, [1..3] detected weight, [4..6] w x the length outside the box, [7] ended (0 here),
[8] detected paths, [9..11] w x the path's length inside the cube, [12] replay disagreements (0: there is no second walk here), [13..15] 0."""
import numpy as np
from tests import lightpath64 as LP
from tests.fluence64 import _slabs, hg_sample, collimated, point, bar, total_bar         # noqa: F401  (re-exported for the tests)
from tests.fluence_track64 import _pieces
from tests.exitance64 import cell as map_cell, normal as map_normal, CUBE


def manual(sigma_s, sigma_a, density, weight):
    """strategy manual: every flight that samples the medium draws t = -log(1 - u) / density"""
    m = LP.homogeneous(sigma_s, sigma_a, "single", weight)
    m["rho"] = float(density)
    return m


def detector(res, face, window, cos_min=0.0, t_min=0.0, t_bin=0.0):
    """res = (res_u, res_v) of the raster, window = (iu0, iu1, iv0, iv1), half-open"""
    return {"res": tuple(res), "face": int(face), "window": tuple(window), "cos_min": float(cos_min), "t_min": float(t_min), "t_bin": float(t_bin)}


def detected(det, xe, de, le):
    """which of the exits (points xe, directions de, optical path lengths le) the detector takes"""
    ok = np.ones(len(xe), bool)
    if det["cos_min"] > 0:
        ok &= ~((de * map_normal(xe, CUBE)).sum(1) < det["cos_min"])
    if det["t_bin"] > 0:
        ok &= np.floor((le - det["t_min"]) / det["t_bin"]) == 0
    ru, rv = det["res"]
    c = map_cell(xe, CUBE, (ru, rv))
    iu, iv, face = c % ru, (c // ru) % rv, c // (ru * rv)
    iu0, iu1, iv0, iv1 = det["window"]
    return ok & (face == det["face"]) & (iu >= iu0) & (iu < iu1) & (iv >= iv0) & (iv < iv1)


def render(emitter, power, medium, g, res, det, bmin=(-1, -1, -1), bmax=(1, 1, 1), n=1.0, paths=4096, batches=16, seed=0, max_depth=-1,
           rr_depth=5, max_events=4096):
    """`batches` independent batches of `paths` paths from `emitter` (geometry only) with the RGB `power` per path:
    (J (batches, nz, ny, nx, 3), totals (batches, 16)), raw sums as the library keeps them"""
    rng = np.random.default_rng(seed)
    power = np.broadcast_to(np.asarray(power, np.float64), (3,))
    ncell = int(np.prod(res))
    homog = medium["kind"] == "homogeneous"
    clear = homog and not medium["st"].any()
    J = np.zeros((batches, ncell, 3)); totals = np.zeros((batches, 16))
    outside = not np.all(np.abs(emitter["o"]) <= 1)
    for b in range(batches):
        N = paths
        L = np.zeros((N, ncell)); Lout = np.zeros(N); Lin = np.zeros(N)      # per path: length per cell, outside the box, inside the cube
        w = np.zeros((N, 3)); hit_det = np.zeros(N, bool)
        pid = np.arange(N)
        x, d = LP._emit(emitter, rng, N)
        T = np.ones((N, 3)); plen = np.zeros(N)
        depth = 1
        if outside:                                                     # to the null boundary: one depth, one roulette trip; the leg deposits nothing
            tn, tf = _slabs(x, d)
            hit = (tn <= tf) & (tn > 0)
            x, d, T, plen, pid = x[hit] + d[hit] * tn[hit, None], d[hit], T[hit], tn[hit] * 1.0, pid[hit]
            if depth >= rr_depth:
                q = np.minimum(T.max(1), 0.95); keep = rng.random(len(T)) < q
                x, d, T, plen, pid = x[keep], d[keep], T[keep] / q[keep, None], plen[keep], pid[keep]
            depth += 1
        for _ in range(max_events):
            if len(T) == 0 or not (depth <= max_depth or max_depth < 0):
                break
            _, tex = _slabs(x, d)
            tfl = np.full(len(T), np.inf) if clear else LP._sample_homogeneous(medium, rng, len(T)) if homog else LP._sample_ramp(medium, rng, x, d)
            sc = tfl < tex
            ex = ~sc
            # ---- the lengths of every flight, collided or not
            fl = np.minimum(tfl, tex)
            pa, pb, idx, inside = _pieces(x, d, fl, res, bmin, bmax)
            rows = np.broadcast_to(pid[:, None], idx.shape)
            np.add.at(L, (rows[inside], idx[inside]), (pb - pa)[inside])
            Lout[pid] += np.where(inside, 0.0, pb - pa).sum(1)
            Lin[pid] += fl
            # ---- the flights that reach the boundary
            we = T[ex] * power
            if homog and not clear:
                tr, _, pf = LP.strategy_pdfs(medium, tex[ex])
                we = we * tr / pf[:, None]
            ok = detected(det, x[ex] + d[ex] * tex[ex, None], d[ex], plen[ex] + tex[ex] * n)
            w[pid[ex][ok]] = we[ok]; hit_det[pid[ex][ok]] = True
            # ---- the collisions
            x, d, T, plen, pid = x[sc] + d[sc] * tfl[sc, None], d[sc], T[sc], plen[sc] + tfl[sc] * n, pid[sc]
            if len(T) == 0:
                break
            if homog:
                tr, ps, _ = LP.strategy_pdfs(medium, tfl[sc])
                T = T * medium["ss"] * tr / ps[:, None]
            else:
                T = T * LP.ramp_albedo(medium, x)
            live = T.max(1) > 0
            x, d, T, plen, pid = x[live], d[live], T[live], plen[live], pid[live]
            d = hg_sample(g, d, rng.random((len(T), 2)))
            if depth >= rr_depth:
                q = np.minimum(T.max(1), 0.95); keep = rng.random(len(T)) < q
                x, d, T, plen, pid = x[keep], d[keep], T[keep] / q[keep, None], plen[keep], pid[keep]
            depth += 1
        wd = w[hit_det]
        J[b] = L[hit_det].T @ wd
        totals[b, 0] = N; totals[b, 1:4] = wd.sum(0); totals[b, 4:7] = Lout[hit_det] @ wd; totals[b, 8] = np.count_nonzero(hit_det)
        totals[b, 9:12] = Lin[hit_det] @ wd
    return J.reshape((batches, res[2], res[1], res[0], 3)), totals
