"""The frequency-domain recorders (include/mer.h, mer_fluence_fd_create / mer_exitance_fd_create) restated in float64 with numpy: two
recorders for lightpath64.walk.  Independent of the library; lightpath64 itself is not touched -- its recorder interface is enough.

GridFD     every real collision adds w (cos, sin)(k_j L) to the cell of the collision point: reads co.x, co.L, co.wdep.
           Raw sums (K, n_freq, 2, nz, ny, nx, C), totals (K, 8) as mer_fluence_fd_read ([4..6]: the plain w of points outside the box).
ExitMapFD  the one exit of a path adds w (cos, sin)(k_j l): reads exits(fl), fl.we and the cone.
           Raw sums (K, n_freq, 2, faces, res_v, res_u, C), totals (K, 16) as mer_exitance_fd_read (no window: [8..10] stay 0).

Scalar (a grey medium: C = 1) or RGB.  k = 0 gives exactly (1, 0): cos(0.0) == 1.0 and sin(0.0) == 0.0 in numpy, so the real plane holds the
steady recorder's sums bit for bit and the imaginary plane stays exactly 0.0."""
import numpy as np
from tests.lightpath64 import (CUBE, Grey, homogeneous, Recorder, cells, cell, faces, normal, exits, _add, walk, collimated, point,      # noqa: F401
                               bar, total_bar)


def _planes(sums_b, ncell, idx, w, L, ks):
    """sums_b (n_freq * 2 * ncell, C) += w (M, C) or (M,) x (cos, sin)(k_j L) at the cells idx"""
    w = w[:, None] if w.ndim == 1 else w
    for j, k in enumerate(ks):
        phi = k * L
        _add(sums_b, (2 * j) * ncell + idx, w * np.cos(phi)[:, None])
        _add(sums_b, (2 * j + 1) * ncell + idx, w * np.sin(phi)[:, None])


class GridFD(Recorder):
    def __init__(self, batches, channels, res, wavenumbers, bmin=(-1, -1, -1), bmax=(1, 1, 1)):
        self.box, self.ncell, self.ks = (res, bmin, bmax), int(np.prod(res)), [float(k) for k in wavenumbers]
        self.shape = (batches, len(self.ks), 2, res[2], res[1], res[0], channels)
        self.sums = np.zeros((batches, len(self.ks) * 2 * self.ncell, channels)); self.totals = np.zeros((batches, 8))

    def collision(self, b, co):
        idx, m = cells(co.x, *self.box)
        self.totals[b, 4:7] += co.wdep[~m].sum(0)
        _planes(self.sums[b], self.ncell, idx[m], co.wdep[m], co.L[m], self.ks)


class ExitMapFD(Recorder):
    def __init__(self, batches, channels, shape, res, wavenumbers, cos_min=0.0):
        self.geo, self.res, self.cos_min, self.ks = shape, res, cos_min, [float(k) for k in wavenumbers]
        self.ncell = faces(shape) * res[0] * res[1]
        self.shape = (batches, len(self.ks), 2, faces(shape), res[1], res[0], channels)
        self.sums = np.zeros((batches, len(self.ks) * 2 * self.ncell, channels)); self.totals = np.zeros((batches, 16))

    def flight(self, b, fl):
        xe, de, le = exits(fl); we = fl.we; t = self.totals[b]
        rej = ((de * normal(xe, self.geo)).sum(1) < self.cos_min) if self.cos_min > 0 else np.zeros(len(we), bool)
        ok = ~rej
        t[11:14] += we[rej].sum(0); t[14] += np.count_nonzero(ok)
        _planes(self.sums[b], self.ncell, cell(xe[ok], self.geo, self.res), we[ok], le[ok], self.ks)

    def end(self, b, paths, escaped, missed):
        Recorder.end(self, b, paths, escaped, missed)
        self.totals[b, 4:7] = missed


def render(emitter, power, medium, g, wavenumbers, grid_res=None, map_res=None, shape=CUBE, cos_min=0.0, n=1.0, paths=4096, batches=16, seed=0,
           max_depth=-1, rr_depth=5):
    """`batches` x `paths` paths through `medium` (Grey: one channel, `power` a scalar; homogeneous: RGB) with both recorders on the same walk:
    {"grid": (K, n_freq, 2, nz, ny, nx, C), "grid_totals": (K, 8), "map": (K, n_freq, 2, faces, rv, ru, C), "map_totals": (K, 16)}"""
    channels = 3 if medium.rgb else 1
    power = np.broadcast_to(np.asarray(power, np.float64), (3,)) if medium.rgb else float(power)
    rec = {}
    if grid_res is not None:
        rec["grid"] = GridFD(batches, channels, grid_res, wavenumbers)
    if map_res is not None:
        rec["map"] = ExitMapFD(batches, channels, shape, map_res, wavenumbers, cos_min)
    walk(emitter, power, shape, medium, g, list(rec.values()), n=n, paths=paths, batches=batches, seed=seed, max_depth=max_depth, rr_depth=rr_depth)
    out = {}
    for key, r in rec.items():
        out[key] = r.result(); out[key + "_totals"] = r.totals
    return out


def absorber_column(power, sigma_a, n, k, a, b, entry=2.0):
    """per path, the complex mean of the cell over the depths [a, b] behind the entry face under an unscattered beam in a pure absorber of
    index n, `entry` units of exterior leg before it: both the deposit P / sigma_a at a first collision of density sigma_a e^{-sigma_a s}
    and its phase k (entry + n s) integrate to P e^{i k entry} (e^{c b} - e^{c a}) / c with c = -sigma_a + i k n"""
    c = -sigma_a + 1j * k * n
    return power * np.exp(1j * k * entry) * (np.exp(c * b) - np.exp(c * a)) / c
