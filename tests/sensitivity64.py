"""The sensitivity grid of mer_render_sensitivity (include/mer.h) restated in float64 with numpy, for a homogeneous RGB medium or the
sigma_t ramp of tests/lightpath64.py (ramp(...): a constant RGB albedo or an albedo grid) with the null boundary in the cube [-1, 1]^3.
Vectorised over the paths of a batch; independent of the library.

The walk is tests/lightpath64.py's (walk, with the media of its render): emitter, one depth and one roulette trip for the null boundary when the emitter lies outside,
free flights by the medium's distance-sampling strategy, the weights transmittance / pdfSuccess at a collision and transmittance /
pdfFailure at the exit, Henyey-Greenstein, roulette.  `manual(...)` adds the strategy the derivative test needs: one exponential of a
FIXED density rho, whatever sigma_t is (Walk::sample_exp_distance with MER_STRATEGY_MANUAL), so that the walks at two values of sigma_a
draw the same paths.  In a ramp the free flights come from lightpath64.ramp.sample (the closed-form inversion of the optical depth), a
collision multiplies T by the ramp's albedo at its point, and a path leaves with T power and no strategy factor.  A homogeneous medium
with sigma_t = 0 is walked as lightpath64.Clear: no draw.

What is new: nothing is deposited while a path walks.  Every flight is cut at the planes of the grid (lightpath64._pieces) and the
lengths of its pieces are added to the path's own row of a dense matrix L[path, cell] (the grids here are small).  A path that leaves
goes through the detector in the expressions of the exitance map -- the cone (cos_min > 0 and d . normal < cos_min: rejected), the gate
(t_bin > 0: detected iff floor((l - t_min) / t_bin) == 0) and the window (the exit's cell lies on `face`, iu0 <= iu < iu1, iv0 <= iv < iv1)
-- and, detected, keeps its weight w.  After the walk J = w^T L over the detected paths.  The recorder (PathMatrices) also serves
tests/sensitivity_array64.py, which reads its measurement index and its collision matrix.

Totals (16, as mer_sensitivity_read): [0] paths, [1..3] detected weight, [4..6] w x the length outside the box, [7] ended (0 here),
[8] detected paths, [9..11] w x the path's length inside the cube, [12] replay disagreements (0: there is no second walk here), [13..15] 0."""
import numpy as np
from tests import lightpath64 as LP
from tests.lightpath64 import CUBE, cells, _pieces, collimated, point, bar, total_bar         # noqa: F401  (re-exported for the tests)


def manual(sigma_s, sigma_a, density, weight):
    """strategy manual: every flight that samples the medium draws t = -log(1 - u) / density"""
    m = LP.homogeneous(sigma_s, sigma_a, "single", weight)
    m.rho = float(density)
    return m


def detector(res, face, window, cos_min=0.0, t_min=0.0, t_bin=0.0):
    """res = (res_u, res_v) of the raster, window = (iu0, iu1, iv0, iv1), half-open"""
    return {"res": tuple(res), "face": int(face), "window": tuple(window), "cos_min": float(cos_min), "t_min": float(t_min), "t_bin": float(t_bin)}


def _bins(det):
    """(bin_u, bin_v): the whole window unless the detector is sensitivity_array64.array's"""
    iu0, iu1, iv0, iv1 = det["window"]
    return det.get("bins") or (max(iu1 - iu0, 1), max(iv1 - iv0, 1))


def shape(det):
    """(gates, ndv, ndu) of a detector: 1 gate unless it is sensitivity_array64.array's"""
    iu0, iu1, iv0, iv1 = det["window"]
    return det.get("gates", 1), (iv1 - iv0) // _bins(det)[1], (iu1 - iu0) // _bins(det)[0]


def measurement(det, xe, de, le):
    """(detected, m) of the exits (points xe, directions de, optical path lengths le): m = (gate ndv + detector row) ndu + detector column"""
    ok = np.ones(len(xe), bool)
    if det["cos_min"] > 0:
        ok &= ~((de * LP.normal(xe, CUBE)).sum(1) < det["cos_min"])
    g = np.zeros(len(xe))
    if det["t_bin"] > 0:
        g = np.floor((le - det["t_min"]) / det["t_bin"])
        ok &= (g >= 0) & (g < det.get("gates", 1))
    ru, rv = det["res"]
    c = LP.cell(xe, CUBE, (ru, rv))
    iu, iv, face = c % ru, (c // ru) % rv, c // (ru * rv)
    iu0, iu1, iv0, iv1 = det["window"]
    ok &= (face == det["face"]) & (iu >= iu0) & (iu < iu1) & (iv >= iv0) & (iv < iv1)
    _, ndv, ndu = shape(det)
    m = (np.where(ok, g, 0).astype(np.int64) * ndv + (iv - iv0) // _bins(det)[1]) * ndu + (iu - iu0) // _bins(det)[0]
    return ok, np.where(ok, m, 0)


def detected(det, xe, de, le):
    """which of the exits the detector takes: `measurement` at its one gate"""
    return measurement(det, xe, de, le)[0]


class PathMatrices(LP.Recorder):
    """per path, dense over the (small) grid: the length L per cell, outside the box (Lout) and inside the cube (Lin); with scatter = True
    also the collisions the path scatters from per cell (C), outside the box (Cout) and in all (Call); the detected weight w and the
    measurement index.  At the end of a batch J[m] = w^T L and K[m] = w^T C over the paths of measurement m.  Only the sensitivity renderers
    attach it: no other renderer pays for the matrices."""

    def __init__(self, batches, res, bmin, bmax, det, scatter=False):
        self.box, self.det, self.scatter, self.ncell = (res, bmin, bmax), det, scatter, int(np.prod(res))
        self.M = int(np.prod(shape(det)))
        self.J = np.zeros((batches, self.M, self.ncell, 3)); self.K = np.zeros((batches, self.M, self.ncell, 3))
        self.meas = np.zeros((batches, self.M, 8)); self.totals = np.zeros((batches, 16))

    def begin(self, b, N):
        self.L = np.zeros((N, self.ncell)); self.Lout = np.zeros(N); self.Lin = np.zeros(N)
        self.C = np.zeros((N, self.ncell if self.scatter else 0)); self.Cout = np.zeros(N); self.Call = np.zeros(N)
        self.w = np.zeros((N, 3)); self.hit = np.zeros(N, bool); self.mof = np.zeros(N, np.int64)

    def flight(self, b, fl):
        # the lengths of every flight, collided or not; the leg outside the shape deposits nothing
        l = np.minimum(fl.tfl, fl.tex)
        pa, pb, idx, inside = _pieces(fl.x, fl.d, l, *self.box)
        rows = np.broadcast_to(fl.pid[:, None], idx.shape)
        np.add.at(self.L, (rows[inside], idx[inside]), (pb - pa)[inside])
        self.Lout[fl.pid] += np.where(inside, 0.0, pb - pa).sum(1)
        self.Lin[fl.pid] += l
        ok, mm = measurement(self.det, *LP.exits(fl))
        p = fl.pid[fl.ex][ok]
        self.w[p] = fl.we[ok]; self.hit[p] = True; self.mof[p] = mm[ok]

    def collision(self, b, co):
        if self.scatter:                                                # the collisions the paths scatter from (T.max() > 0 afterwards)
            pid = co.pid[co.live]
            cc, cin = cells(co.x[co.live], *self.box)
            self.Call[pid] += 1.0
            np.add.at(self.C, (pid[cin], cc[cin]), 1.0)
            self.Cout[pid[~cin]] += 1.0

    def end(self, b, paths, escaped, missed):
        for m in range(self.M):
            sel = self.hit & (self.mof == m)
            wd = self.w[sel]
            self.J[b, m] = self.L[sel].T @ wd
            if self.scatter:
                self.K[b, m] = self.C[sel].T @ wd
            self.meas[b, m, 0:3] = wd.sum(0); self.meas[b, m, 3] = np.count_nonzero(sel); self.meas[b, m, 4:7] = self.Call[sel] @ wd
        wd = self.w[self.hit]; t = self.totals[b]
        t[0] = paths; t[1:4] = wd.sum(0); t[4:7] = self.Lout[self.hit] @ wd; t[8] = np.count_nonzero(self.hit)
        t[9:12] = self.Lin[self.hit] @ wd; t[13:16] = self.Cout[self.hit] @ wd


def record(emitter, power, medium, g, res, det, bmin, bmax, scatter, **kw):
    """the walk of sensitivity64.render and sensitivity_array64.render with the per-path matrices attached: the recorder"""
    if isinstance(medium, LP.homogeneous) and not medium.st.any():
        medium = LP.Clear()
    rec = PathMatrices(kw["batches"], res, bmin, bmax, det, scatter)
    LP.walk(emitter, np.broadcast_to(np.asarray(power, np.float64), (3,)), CUBE, medium, g, [rec], **kw)
    return rec


def render(emitter, power, medium, g, res, det, bmin=(-1, -1, -1), bmax=(1, 1, 1), n=1.0, paths=4096, batches=16, seed=0, max_depth=-1,
           rr_depth=5, max_events=4096):
    """`batches` independent batches of `paths` paths from `emitter` (geometry only) with the RGB `power` per path:
    (J (batches, nz, ny, nx, 3), totals (batches, 16)), raw sums as the library keeps them"""
    rec = record(emitter, power, medium, g, res, det, bmin, bmax, False, n=n, paths=paths, batches=batches, seed=seed, max_depth=max_depth,
                 rr_depth=rr_depth, max_events=max_events)
    return rec.J[:, 0].reshape((batches, res[2], res[1], res[0], 3)), rec.totals
