"""The sensitivity grids of an array of detectors and gates (mer_sensitivity_array_create, include/mer.h) restated in float64 with numpy: the
walk of tests/sensitivity64.py (render), draw for draw -- the same calls on the same generator in the same order, so that one seed walks the
same paths in both -- with two additions per path:

  the measurement  a path that leaves through raster cell (iu, iv) of the window in gate g = floor((l - t_min) / t_bin), 0 <= g < gates,
                   past the cone, belongs to m = (g ndv + (iv - iv0) // bin_v) ndu + (iu - iu0) // bin_u (gates = 1 and t_bin = 0: no gate);
  the collisions   every collision the path scatters from (it survives the albedo: T.max() > 0 afterwards, as LightPath::collide returns
                   true) adds 1 to the path's row of a dense matrix N[path, cell] at the cell of the collision point, or to the path's
                   count outside the box; the path's count of all of them is kept apart, before any box test.

After the walk, per measurement: J[m] = w^T L and K[m] = w^T N over the paths of m.

Returns J and K (batches, gates, ndv, ndu, nz, ny, nx, 3), meas (batches, gates, ndv, ndu, 8: detected weight x 3, detected paths,
w x collisions x 3, 0) and totals (batches, 16: as sensitivity64.render over all measurements; [13..15] w per collision outside the box)."""
import numpy as np
from tests import sensitivity64 as S
from tests import lightpath64 as LP
from tests.fluence64 import _slabs, hg_sample
from tests.fluence_track64 import _pieces
from tests.exitance64 import cell as map_cell, normal as map_normal, CUBE


def array(res, face, window, bins=None, gates=1, cos_min=0.0, t_min=0.0, t_bin=0.0):
    """the detector dict of sensitivity64.detector plus bins = (bin_u, bin_v) (None: the whole window) and the gates"""
    d = S.detector(res, face, window, cos_min, t_min, t_bin)
    iu0, iu1, iv0, iv1 = d["window"]
    d["bins"] = (iu1 - iu0, iv1 - iv0) if bins is None else tuple(int(v) for v in bins)
    d["gates"] = int(gates)
    assert (iu1 - iu0) % d["bins"][0] == 0 and (iv1 - iv0) % d["bins"][1] == 0 and gates >= 1 and (gates == 1 or t_bin > 0)
    return d


def shape(det):
    iu0, iu1, iv0, iv1 = det["window"]
    return det["gates"], (iv1 - iv0) // det["bins"][1], (iu1 - iu0) // det["bins"][0]


def measurement(det, xe, de, le):
    """(detected, m) of the exits (points xe, directions de, optical path lengths le)"""
    ok = np.ones(len(xe), bool)
    if det["cos_min"] > 0:
        ok &= ~((de * map_normal(xe, CUBE)).sum(1) < det["cos_min"])
    g = np.zeros(len(xe))
    if det["t_bin"] > 0:
        g = np.floor((le - det["t_min"]) / det["t_bin"])
        ok &= (g >= 0) & (g < det["gates"])
    ru, rv = det["res"]
    c = map_cell(xe, CUBE, (ru, rv))
    iu, iv, face = c % ru, (c // ru) % rv, c // (ru * rv)
    iu0, iu1, iv0, iv1 = det["window"]
    ok &= (face == det["face"]) & (iu >= iu0) & (iu < iu1) & (iv >= iv0) & (iv < iv1)
    _, ndv, ndu = shape(det)
    m = (np.where(ok, g, 0).astype(np.int64) * ndv + (iv - iv0) // det["bins"][1]) * ndu + (iu - iu0) // det["bins"][0]
    return ok, np.where(ok, m, 0)


def point_cell(x, res, bmin, bmax):
    """(inside, cell) of the points x: per axis floor((p - bmin) / (bmax - bmin) res), half-open (fluence_cell)"""
    lo, hi, n = np.asarray(bmin, np.float64), np.asarray(bmax, np.float64), np.asarray(res)
    f = np.floor((x - lo) / (hi - lo) * n)
    inside = np.all((f >= 0) & (f < n), 1)
    i = np.where(inside[:, None], f, 0).astype(np.int64)
    return inside, (i[:, 2] * res[1] + i[:, 1]) * res[0] + i[:, 0]


def render(emitter, power, medium, g, res, det, bmin=(-1, -1, -1), bmax=(1, 1, 1), n=1.0, paths=4096, batches=16, seed=0, max_depth=-1,
           rr_depth=5, max_events=4096):
    """`batches` independent batches of `paths` paths: (J, K, meas, totals), raw sums as the library keeps them"""
    rng = np.random.default_rng(seed)
    power = np.broadcast_to(np.asarray(power, np.float64), (3,))
    ncell = int(np.prod(res))
    gates, ndv, ndu = shape(det)
    M = gates * ndv * ndu
    homog = medium["kind"] == "homogeneous"
    clear = homog and not medium["st"].any()
    J = np.zeros((batches, M, ncell, 3)); K = np.zeros((batches, M, ncell, 3)); meas = np.zeros((batches, M, 8)); totals = np.zeros((batches, 16))
    outside = not np.all(np.abs(emitter["o"]) <= 1)
    for b in range(batches):
        N = paths
        L = np.zeros((N, ncell)); Lout = np.zeros(N); Lin = np.zeros(N)      # per path: length per cell, outside the box, inside the cube
        C = np.zeros((N, ncell)); Cout = np.zeros(N); Call = np.zeros(N)      # per path: collisions per cell, outside the box, all
        w = np.zeros((N, 3)); hit_det = np.zeros(N, bool); mof = np.zeros(N, np.int64)
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
            ok, mm = measurement(det, x[ex] + d[ex] * tex[ex, None], d[ex], plen[ex] + tex[ex] * n)
            w[pid[ex][ok]] = we[ok]; hit_det[pid[ex][ok]] = True; mof[pid[ex][ok]] = mm[ok]
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
            # the collisions the paths scatter from: counted, then put into the cell of the collision point
            cin, cc = point_cell(x, res, bmin, bmax)
            Call[pid] += 1.0
            np.add.at(C, (pid[cin], cc[cin]), 1.0)
            Cout[pid[~cin]] += 1.0
            d = hg_sample(g, d, rng.random((len(T), 2)))
            if depth >= rr_depth:
                q = np.minimum(T.max(1), 0.95); keep = rng.random(len(T)) < q
                x, d, T, plen, pid = x[keep], d[keep], T[keep] / q[keep, None], plen[keep], pid[keep]
            depth += 1
        for m in range(M):
            sel = hit_det & (mof == m)
            wd = w[sel]
            J[b, m] = L[sel].T @ wd
            K[b, m] = C[sel].T @ wd
            meas[b, m, 0:3] = wd.sum(0); meas[b, m, 3] = np.count_nonzero(sel); meas[b, m, 4:7] = Call[sel] @ wd
        wd = w[hit_det]
        totals[b, 0] = N; totals[b, 1:4] = wd.sum(0); totals[b, 4:7] = Lout[hit_det] @ wd; totals[b, 8] = np.count_nonzero(hit_det)
        totals[b, 9:12] = Lin[hit_det] @ wd; totals[b, 13:16] = Cout[hit_det] @ wd
    grid = (batches, gates, ndv, ndu, res[2], res[1], res[0], 3)
    return J.reshape(grid), K.reshape(grid), meas.reshape((batches, gates, ndv, ndu, 8)), totals
